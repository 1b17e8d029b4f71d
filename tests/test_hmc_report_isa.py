"""Register metadata of the hedge-report kernels (psh_hmc_report.hip), read from the compiler's own output (hipcc -S for
gfx950, no GPU needed): no instantiation -- the fit with its policy kept, the replay, the final sum -- spills or touches
scratch memory."""
import re
import subprocess

from shadowing_amd import _build


def test_report_kernels_do_not_spill(tmp_path):
    out = tmp_path / "psh_hmc_report.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_hmc_report.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in out.read_text().split("  - .agpr_count:")[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        meta[g("name")] = dict(spill=int(g("vgpr_spill_count")), scratch=int(g("private_segment_fixed_size")))
    for stem, count in (("hmc_policy_kernel", 5), ("hedge_replay_kernel", 5), ("hedge_finish_kernel", 1)):   # degrees 1..5
        assert sum(stem in n for n in meta) == count, meta
    assert len(meta) == 11, meta
    assert all(m["spill"] == 0 and m["scratch"] == 0 for m in meta.values()), meta
