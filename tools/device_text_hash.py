#!/usr/bin/env python3
"""sha256 of the gfx950 device code (.text) of every HIP source of the library.  CPU only, needs no GPU.

    python tools/device_text_hash.py [--csrc DIR] [extra compiler flags, e.g. -DCT_EXPERIMENTS]

Each .hip file of build.SOURCES is compiled for the device alone with build.FLAGS, its gfx950 code object is taken out of
the bundle and the .text section is hashed.  Two trees whose lines are equal pairwise run the same kernels: this is how a
change that is meant to leave the device code alone (comments, dead switches, line numbers) is shown to do so.
--csrc names the csrc directory of another checkout to hash, e.g. an export of the parent commit.
"""
from __future__ import annotations

import hashlib
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from deepestscatter_amd import build  # noqa: E402

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def device_text_sha256(src: Path, extra: list[str], tmp: Path) -> str:
    hipcc = build.hipcc()
    llvm = Path(hipcc).resolve().parent.parent / "llvm" / "bin"
    if not (llvm / "clang-offload-bundler").exists():
        llvm = Path("/opt/rocm/llvm/bin")
    bundle, co, text = tmp / "bundle.o", tmp / "gfx950.co", tmp / "text.bin"
    flags = [f for f in build.FLAGS if f != "-shared"]
    subprocess.run([hipcc, *flags, *extra, "--offload-device-only", "-c", "-o", str(bundle), src.name], check=True, cwd=str(src.parent))
    subprocess.run([str(llvm / "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                    f"--input={bundle}", f"--output={co}"], check=True)
    subprocess.run([str(llvm / "llvm-objcopy"), f"--dump-section=.text={text}", str(co)], check=True)
    return hashlib.sha256(text.read_bytes()).hexdigest()


def main(argv: list[str]) -> int:
    csrc = build.CSRC
    if "--csrc" in argv:
        i = argv.index("--csrc")
        csrc = Path(argv[i + 1]).resolve()
        argv = argv[:i] + argv[i + 2:]
    with tempfile.TemporaryDirectory() as tmp:
        for name in build.SOURCES:
            if name.endswith(".hip"):
                print(f"{device_text_sha256(csrc / name, argv, Path(tmp))}  {name}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
