"""Register and LDS metadata of the separation kernels (psh_separate.hip), read from the compiler's own output (hipcc -S for
gfx950, no GPU needed): the instantiations are counted, none spills or touches scratch memory, and each fits the LDS one
workgroup may hold -- the largest holds 16384 padded entries and their state bytes with less than 8 KiB beside them."""
import re
import subprocess

from shadowing_amd import _build

LDS_PER_WORKGROUP = 163840


def test_separation_kernels_do_not_spill_and_fit_lds(tmp_path):
    out = tmp_path / "psh_separate.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_separate.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in out.read_text().split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        meta[g("name")] = dict(spill=int(g("vgpr_spill_count")), scratch=int(g("private_segment_fixed_size")),
                               lds=int(g("group_segment_fixed_size")))
    sk = {n: m for n, m in meta.items() if "separate_kernel" in n}
    assert len(sk) == len(meta) == 3, meta                        # capacities 1024, 4096 and 16384 entries
    assert all(m["spill"] == 0 and m["scratch"] == 0 for m in sk.values()), sk
    lds = sorted(m["lds"] for m in sk.values())
    assert lds[-1] <= LDS_PER_WORKGROUP, sk
    for have, cap in zip(lds, (1024, 4096, 16384)):               # each holds its padded entries and a state byte per entry
        working = (cap + cap // 16) * 8 + cap
        assert working <= have <= working + 8192, sk
    assert 4 * lds[0] <= LDS_PER_WORKGROUP, sk                    # four workgroups of the smallest on a compute unit


def test_the_library_is_built_from_the_new_translation_unit():
    assert _build.CSRC / "psh_separate.hip" in _build.SOURCES
