"""Register metadata of the PDV path generator (psh_pdv.hip), read from the compiler's own output (hipcc -S for gfx950, no
GPU needed): no instantiation spills or touches scratch memory."""
import re
import subprocess

from shadowing_amd import _build


def test_pdv_kernel_does_not_spill(tmp_path):
    out = tmp_path / "psh_pdv.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_pdv.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in out.read_text().split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        meta[g("name")] = dict(spill=int(g("vgpr_spill_count")), scratch=int(g("private_segment_fixed_size")))
    pdv = {n: m for n, m in meta.items() if "pdv_kernel" in n}
    assert len(pdv) == 6, meta                                   # Gaussian / Student-t / given draws x 3 or 4 betas
    assert all(m["spill"] == 0 and m["scratch"] == 0 for m in pdv.values()), pdv
