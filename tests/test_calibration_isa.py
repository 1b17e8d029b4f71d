"""Register and LDS metadata of the calibration kernels (psh_calibrate.hip), read from the compiler's own output (hipcc -S
for gfx950, no GPU needed): the Newton kernel, whose loop is the whole kernel, holds no scratch memory and spills no vector
register, and its LDS -- the tile of h, the two J x J matrices -- fits what one workgroup may hold."""
import re
import subprocess

from shadowing_amd import _build

LDS_PER_WORKGROUP = 163840


def test_calibration_kernels_hold_no_scratch_and_fit_lds(tmp_path):
    out = tmp_path / "psh_calibrate.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_calibrate.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in out.read_text().split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        meta[g("name")] = dict(spill=int(g("vgpr_spill_count")), scratch=int(g("private_segment_fixed_size")),
                               lds=int(g("group_segment_fixed_size")), vgpr=int(g("vgpr_count")))
    newton = [m for n, m in meta.items() if "cal_newton_kernel" in n]
    terminal = [m for n, m in meta.items() if "cal_terminal_kernel" in n]
    assert len(newton) == len(terminal) == 1 and len(meta) == 2, meta
    assert all(m["spill"] == 0 and m["scratch"] == 0 for m in meta.values()), meta
    assert 32 * 512 * 8 <= newton[0]["lds"] <= LDS_PER_WORKGROUP, meta      # the tile of 512 paths x 32 instruments and the rest
    assert newton[0]["vgpr"] <= 256 and terminal[0]["lds"] == 256 * 33 * 4, meta   # 512 threads a workgroup: 256 registers each


def test_the_library_is_built_from_the_new_translation_unit():
    assert _build.CSRC / "psh_calibrate.hip" in _build.SOURCES and _build.CSRC / "psh_calibrate.hip" in _build.DEPS
