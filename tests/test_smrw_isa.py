"""Register and LDS metadata of the skewed MRW generator (psh_smrw.hip), read from the compiler's own output (hipcc -S for
gfx950, no GPU needed): no instantiation spills or touches scratch memory, and each fits the LDS one workgroup may
hold."""
import re
import subprocess

from shadowing_amd import _build

LDS_PER_WORKGROUP = 163840


def test_smrw_kernels_do_not_spill_and_fit_lds(tmp_path):
    out = tmp_path / "psh_smrw.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_smrw.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in out.read_text().split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        meta[g("name")] = dict(spill=int(g("vgpr_spill_count")), scratch=int(g("private_segment_fixed_size")),
                               lds=int(g("group_segment_fixed_size")))
    smrw = {n: m for n, m in meta.items() if "smrw" in n}
    assert len(smrw) == 2, meta                                  # M <= 2048 / M <= 8192
    assert all(m["spill"] == 0 and m["scratch"] == 0 for m in smrw.values()), smrw
    assert all(0 < m["lds"] <= LDS_PER_WORKGROUP for m in smrw.values()), smrw
    assert max(m["lds"] for m in smrw.values()) >= 8192 * 16    # the M = 8192 transform is held whole


def test_the_library_is_built_from_the_new_translation_unit():
    assert _build.CSRC / "psh_smrw.hip" in _build.SOURCES
    assert _build.CSRC / "psh_mrw_lds.h" in _build.DEPS          # a change of the shared transform rebuilds the library
