"""Register and LDS metadata of the scattering gradient kernels (psh_scattering_grad.hip), read from the compiler's own
output (hipcc -S for gfx950, no GPU needed): no kernel spills a vector register or touches scratch memory, each fits the LDS
one workgroup may hold, the n <= 4096 instantiation holds the working buffer and the kept envelope spectra whole, and the
n <= 1024 one needs a quarter of it."""
import re
import subprocess

from shadowing_amd import _build

LDS_PER_WORKGROUP = 163840


def test_scattering_gradient_kernels_do_not_spill_and_fit_lds(tmp_path):
    out = tmp_path / "psh_scattering_grad.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_scattering_grad.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in out.read_text().split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        meta[g("name")] = dict(spill=int(g("vgpr_spill_count")), scratch=int(g("private_segment_fixed_size")),
                               lds=int(g("group_segment_fixed_size")))
    grad = {n: m for n, m in meta.items() if "scatgrad_kernel" in n}
    assert len(grad) == 2 and len(meta) == 3, meta               # n <= 1024 / n <= 4096, and the status fold
    assert not any("scat_kernel" in n for n in meta)             # (tests/test_scattering_isa.py counts those names)
    assert all(m["spill"] == 0 and m["scratch"] == 0 for m in meta.values()), meta
    assert all(m["lds"] <= LDS_PER_WORKGROUP for m in meta.values()), meta
    small, large = sorted(m["lds"] for m in grad.values())
    # the working buffer (64 KiB) and the kept envelope spectra (48 KiB) are held whole at n = 4096
    assert large >= 4096 * 16 + 3072 * 16
    assert 0 < small < large and small < 65536                   # the small instantiation leaves room for more workgroups
