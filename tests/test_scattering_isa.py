"""Register and LDS metadata of the scattering kernel (psh_scattering.hip), read from the compiler's own output (hipcc -S
for gfx950, no GPU needed): no instantiation spills or touches scratch memory, each fits the LDS one workgroup may hold,
and the largest holds the working buffer of 4096 complex doubles whole."""
import re
import subprocess

from shadowing_amd import _build

LDS_PER_WORKGROUP = 163840


def test_scattering_kernels_do_not_spill_and_fit_lds(tmp_path):
    out = tmp_path / "psh_scattering.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_scattering.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in out.read_text().split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        meta[g("name")] = dict(spill=int(g("vgpr_spill_count")), scratch=int(g("private_segment_fixed_size")),
                               lds=int(g("group_segment_fixed_size")))
    scat = {n: m for n, m in meta.items() if "scat_kernel" in n}
    assert len(scat) == 2, meta                                  # n <= 1024 / n <= 4096
    assert all(m["spill"] == 0 and m["scratch"] == 0 for m in meta.values()), meta      # the reduction as well
    assert all(0 < m["lds"] <= LDS_PER_WORKGROUP for m in scat.values()), scat
    # the working buffer (64 KiB), F[x] (32 KiB) and the kept envelope spectra (32 KiB) are held whole at n = 4096
    assert max(m["lds"] for m in scat.values()) >= 4096 * 16 + 2 * 2048 * 16
    assert min(m["lds"] for m in scat.values()) < 65536          # the small instantiation leaves room for more workgroups


def test_the_library_is_built_from_the_new_translation_unit():
    assert _build.CSRC / "psh_scattering.hip" in _build.SOURCES
    assert _build.CSRC / "psh_mrw_lds.h" in _build.DEPS          # the forward transform it shares with the generators
    assert _build.CSRC / "psh_kernels.h" in _build.DEPS and _build.INCLUDE / "psh.h" in _build.DEPS
