"""Register metadata of the f16 filter copy's kernels, read from the compiler's own output as tests/test_isa_metadata.py reads
it: the copy scan fits the 112 registers stream_scan_kernel has (a sample or ranking wave of another stream's step still fits
beside four of its waves on a SIMD), its W = 20 instantiation neither spills nor touches scratch, the build does not spill."""
import pytest

from test_isa_metadata import _asm, _kernels


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return _kernels(_asm("psh_stream_copy", tmp_path_factory.mktemp("isa_copy")))


def test_copy_scan_fits_beside_a_sample_wave(kernels):
    scan = {n: m for n, m in kernels.items() if "copy_scan_kernel" in n}
    assert len(scan) == 2, sorted(kernels)
    assert all(m["vgpr"] <= 112 for m in scan.values()), scan
    w20 = [m for n, m in scan.items() if "ILi20E" in n]
    assert len(w20) == 1 and w20[0]["spill"] == 0 and w20[0]["scratch"] == 0, scan
    # the names the existing ISA tests count and bound stay theirs
    assert not any(s in n for n in kernels for s in ("stream_scan_kernel", "scan_fused_kernel", "stream_scan_long_kernel"))


def test_build_kernels_do_not_spill(kernels):
    build = {n: m for n, m in kernels.items() if any(s in n for s in ("copy_sumsq_kernel", "copy_exponent_kernel", "copy_write_kernel"))}
    assert len(build) == 3, sorted(kernels)
    assert all(m["spill"] == 0 and m["scratch"] == 0 for m in build.values()), build
