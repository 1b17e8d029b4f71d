"""copy_scan_kernel (psh_stream_copy.hip) loads its A fragments straight from the resident f16 copy: lane (m = lane & 31,
hk = lane >> 5) reads, for K-step s, the eight halves [32 m + 16 s + 8 hk, + 8) of the segment with ONE 16-byte load.  Restated
here in numpy for every (lane, s) of every segment: each address is 16-byte aligned and inside its row, a segment's fragments
cover exactly [seg_start, seg_start + 1056) -- and what the compiler made of the kernel spills nothing and keeps four waves
per SIMD (no GPU needed: hipcc cross-compiles for gfx950)."""
import re
import subprocess

import numpy as np
import pytest

from shadowing_amd import _build, _native

SEG, HDR_BYTES = 1024, 64
W, H = 20, 20


@pytest.mark.parametrize("T", [W + H, 1023, 1024, 1025, 2299, 4096])
def test_fragment_addresses(T):
    R = 3
    nbytes, pitch = _native.filter_copy_bytes(R, T)
    assert nbytes == HDR_BYTES + R * pitch * 2 and pitch % 32 == 0
    Tp = T - W - H + 1
    nseg = (Tp + SEG - 1) // SEG
    lane = np.arange(64)
    m, hk = lane & 31, lane >> 5
    s = np.arange(4)
    first = (32 * m[:, None] + 16 * s[None, :] + 8 * hk[:, None]).ravel()       # first half of a fragment, in the segment
    for row in range(R):
        for sg in range(nseg):
            seg_start = sg * SEG
            half0 = seg_start + first                                            # ... in the row
            byte0 = HDR_BYTES + 2 * (row * pitch + half0)                       # ... from the start of the allocation
            assert (byte0 % 16 == 0).all()
            assert (half0 >= 0).all() and (half0 + 8 <= pitch).all(), (T, sg, int(half0.max()) + 8, pitch)
            assert (byte0 + 16 <= nbytes).all()
            count = np.zeros(pitch, dtype=np.int64)
            for h0 in half0:
                count[h0:h0 + 8] += 1
            want = np.zeros(pitch, dtype=np.int64)
            want[seg_start:seg_start + SEG + 32] = 1
            want[seg_start + 32:seg_start + SEG] = 2
            assert np.array_equal(count, want), (T, row, sg)


def test_copy_scan_kernel_keeps_its_registers(tmp_path):
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", str(_build.CSRC / "psh_stream_copy.hip"),
                          "-o", str(tmp_path / "psh_stream_copy.s")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    meta = {}
    for blk in res.stderr.split("Function Name: ")[1:]:
        name = blk.split()[0]
        g = lambda k: int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1))   # noqa: E731
        meta[name] = dict(scratch=g("ScratchSize [bytes/lane]"), spill=g("VGPRs Spill"), occupancy=g("Occupancy [waves/SIMD]"))
    scans = {n: v for n, v in meta.items() if "copy_scan_kernel" in n}
    assert len(scans) == 2, meta                                                 # copy_scan_kernel<20>, copy_scan_kernel<0>
    for n, v in scans.items():
        assert v == dict(scratch=0, spill=0, occupancy=4), (n, v)
