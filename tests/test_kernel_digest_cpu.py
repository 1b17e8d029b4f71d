"""tools/kernel_digest.py on one small unit (hipcc -S for gfx950, no GPU needed): every kernel the metadata lists gets a
hash of its body, the hash does not move when the compiler numbers its local labels differently or a comment changes, and
does move with an instruction."""
import re
import subprocess
import sys
from pathlib import Path

import pytest

from shadowing_amd import _build

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
import kernel_digest  # noqa: E402


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("digest") / "psh_hmc.s"
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S", "--cuda-device-only",
                          str(_build.CSRC / "psh_hmc.hip"), "-o", str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return out.read_text()


def test_every_kernel_is_hashed_with_its_metadata(asm):
    d = kernel_digest.digest_asm(asm)
    kernels = [n for n in d if "hmc_kernel" in n]
    assert len(kernels) == 5                                           # degrees 1 .. 5
    for name in kernels:
        assert re.fullmatch(r"[0-9a-f]{64}", d[name]["sha256"]) and set(kernel_digest.META) <= set(d[name]), name
    assert len({d[n]["sha256"] for n in kernels}) == 5


def test_the_hash_ignores_label_numbers_and_comments_and_sees_instructions(asm):
    d = kernel_digest.digest_asm(asm)
    renumbered = re.sub(r"\.LBB(\d+)_", lambda m: f".LBB{int(m.group(1)) + 7}_", asm).replace("; %bb.", "; block ")
    assert renumbered != asm and kernel_digest.digest_asm(renumbered) == d
    edited = asm.replace("s_endpgm", "s_nop 0\n\ts_endpgm", 1)
    changed = [n for n, e in kernel_digest.digest_asm(edited).items() if e != d[n]]
    assert len(changed) == 1


def test_a_listed_kernel_without_a_body_is_an_error(asm):
    with pytest.raises(RuntimeError, match="no function body"):
        kernel_digest.digest_asm(asm.replace("; -- Begin function", "; -- begin function"))
