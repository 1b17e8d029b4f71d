"""Register and LDS metadata of the lagged-moments kernels (psh_moments.hip), read from the compiler's own output (hipcc -S
for gfx950, no GPU needed): no kernel spills or touches scratch memory, and each fits the LDS one workgroup may hold."""
import re
import subprocess

from shadowing_amd import _build

LDS_PER_WORKGROUP = 163840


def test_moments_kernels_do_not_spill_and_fit_lds(tmp_path):
    out = tmp_path / "psh_moments.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_moments.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in out.read_text().split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        meta[g("name")] = dict(spill=int(g("vgpr_spill_count")), scratch=int(g("private_segment_fixed_size")),
                               lds=int(g("group_segment_fixed_size")))
    mom = {n: m for n, m in meta.items() if "moments" in n}
    assert len(mom) == 4, meta                                   # 1, 2 and 4 lags per lane, and the sum of the partials
    assert all(m["spill"] == 0 and m["scratch"] == 0 for m in mom.values()), mom
    assert all(m["lds"] <= LDS_PER_WORKGROUP for m in mom.values()), mom
    assert sum(m["lds"] > 0 for m in mom.values()) == 3          # the three that stage a tile


def test_the_library_is_built_from_the_new_translation_unit():
    assert _build.CSRC / "psh_moments.hip" in _build.SOURCES
