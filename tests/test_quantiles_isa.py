"""Register and LDS metadata of the quantile kernels (psh_quantiles.hip), read from the compiler's own output (hipcc -S for
gfx950, no GPU needed): the instantiations are counted, none spills or touches scratch memory, each fits the LDS one
workgroup may hold, and the smallest leaves room for four workgroups on a compute unit."""
import re
import subprocess

from shadowing_amd import _build

LDS_PER_WORKGROUP = 163840


def test_quantile_kernels_do_not_spill_and_fit_lds(tmp_path):
    out = tmp_path / "psh_quantiles.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_quantiles.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in out.read_text().split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        meta[g("name")] = dict(spill=int(g("vgpr_spill_count")), scratch=int(g("private_segment_fixed_size")),
                               lds=int(g("group_segment_fixed_size")))
    qk = {n: m for n, m in meta.items() if "quantiles_kernel" in n}
    assert len(qk) == len(meta) == 3, meta                        # capacities 1024, 4096 and 16384 entries
    assert all(m["spill"] == 0 and m["scratch"] == 0 for m in qk.values()), qk
    lds = sorted(m["lds"] for m in qk.values())
    assert lds[-1] <= LDS_PER_WORKGROUP, qk
    assert lds[0] >= 1024 * 8 and lds[1] >= 4096 * 8 and lds[2] >= 16384 * 8, qk      # each holds its entries
    assert 4 * lds[0] <= LDS_PER_WORKGROUP, qk                    # four workgroups of the smallest on a compute unit


def test_the_library_is_built_from_the_new_translation_unit():
    assert _build.CSRC / "psh_quantiles.hip" in _build.SOURCES
