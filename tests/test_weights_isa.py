"""Register and LDS metadata of the weights kernels (psh_weights.hip), read from the compiler's own output (hipcc -S for
gfx950, no GPU needed): one instantiation per capacity, none spills or touches scratch memory, each holds its entries and
fits the LDS one workgroup may hold."""
import re
import subprocess

from shadowing_amd import _build

LDS_PER_WORKGROUP = 163840


def test_weights_kernels_do_not_spill_and_fit_lds(tmp_path):
    out = tmp_path / "psh_weights.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_weights.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in out.read_text().split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        meta[g("name")] = dict(spill=int(g("vgpr_spill_count")), sspill=int(g("sgpr_spill_count")),
                               scratch=int(g("private_segment_fixed_size")), lds=int(g("group_segment_fixed_size")))
    wk = {n: m for n, m in meta.items() if "weights_kernel" in n}
    assert len(wk) == len(meta) == 3, meta                        # capacities 1024, 4096 and 16384 entries
    assert all(m["spill"] == 0 and m["sspill"] == 0 and m["scratch"] == 0 for m in wk.values()), wk
    lds = sorted(m["lds"] for m in wk.values())
    assert lds[-1] <= LDS_PER_WORKGROUP, wk
    assert lds[0] >= 1024 * 8 and lds[1] >= 4096 * 8 and lds[2] >= 16384 * 8, wk      # each holds its entries
    assert 4 * lds[0] <= LDS_PER_WORKGROUP, wk                    # four workgroups of the smallest on a compute unit


def test_the_library_is_built_from_the_new_translation_unit_and_the_shared_header():
    assert _build.CSRC / "psh_weights.hip" in _build.SOURCES
    assert _build.CSRC / "psh_weights.hip" in _build.DEPS and _build.CSRC / "psh_sort_lds.h" in _build.DEPS
