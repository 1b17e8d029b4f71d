"""Digest of every compiled device function, to compare two checkouts' kernels without a GPU.

For each unit of _build.SOURCES: hipcc -S --cuda-device-only under the build's own flags, the assembly split at the
compiler's "Begin function" / "End function" marks, comments dropped, the numbers the compiler gives its local labels
replaced (they count functions in order of instantiation), and what is left hashed.  Beside the hash go the kernel's
metadata fields.  The order of functions in a file follows the order of instantiation, so two files can differ while every
function in them is the same: compare the JSON this writes, not the assembly.

    python tools/kernel_digest.py out.json [unit.hip ...]
"""
from __future__ import annotations

import hashlib
import json
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from shadowing_amd import _build  # noqa: E402

META = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size")
LOCAL_LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp|LJTI|LCPI)\d+")
# (the begin mark trails the function's .protected line, the end mark stands on a line of its own behind spaces)
FUNCTION = re.compile(r"; -- Begin function (\S+)\n(.*?); -- End function", re.S)


def digest_asm(asm: str) -> dict:
    """{function: {"sha256": ..., metadata fields...}} of one unit's device assembly."""
    out = {}
    for name, body in FUNCTION.findall(asm):
        lines = (LOCAL_LABEL.sub(r".\1#", ln.split(";", 1)[0]).rstrip() for ln in body.splitlines())
        out[name] = {"sha256": hashlib.sha256("\n".join(ln for ln in lines if ln).encode()).hexdigest()}
    for blk in asm.split("  - .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        field = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)   # noqa: E731
        out.setdefault(field("name"), {}).update({k: int(field(k)) for k in META})
    unhashed = sorted(name for name, entry in out.items() if "sha256" not in entry)
    if unhashed:         # a kernel the metadata lists but no pair of marks encloses: the marks' format has changed
        raise RuntimeError(f"no function body found for {unhashed}")
    return out


def digest_unit(src: Path) -> dict:
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        asm = Path(tmp) / (src.stem + ".s")
        res = subprocess.run([_build.hipcc_path(), *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "-S",
                              "--cuda-device-only", str(src), "-o", str(asm)], capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src.name}:\n{res.stderr[-4000:]}")
        return digest_asm(asm.read_text())


def main(argv: list[str]) -> int:
    if not argv:
        print(__doc__)
        return 2
    units = [_build.CSRC / a for a in argv[1:]] or _build.SOURCES
    with ThreadPoolExecutor(max_workers=8) as pool:
        digests = dict(zip((u.name for u in units), pool.map(digest_unit, units)))
    if not any(digests.values()):
        raise RuntimeError("no device function found in any unit")
    Path(argv[0]).write_text(json.dumps(digests, indent=1, sort_keys=True) + "\n")
    print(f"{sum(len(d) for d in digests.values())} functions hashed in {len(digests)} units -> {argv[0]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
