"""sha256 of each .hip file's device code object -- the proof that a change left the device code
alone.  Every file is compiled as the library builds it (build.FLAGS and build.FILE_FLAGS), device
side only and with a fixed -cuid, into a temporary directory; equal hashes before and after a change
mean byte-identical kernels.  CPU only: nothing here touches a GPU.

    python tools/code_object_hash.py              # every encdiff_amd/csrc/*.hip
    python tools/code_object_hash.py gemm norm    # only these (name, file name or path)

Prints "name  first 16 hex digits" per file, sorted by name.
"""
from __future__ import annotations

import concurrent.futures as cf
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from encdiff_amd import build  # noqa: E402

CUID = "encdiff"


def code_object_hash(src: str, tmp: str) -> str:
    name = os.path.basename(src)
    out = os.path.join(tmp, name + ".co")
    cmd = [build.HIPCC, *build.FLAGS, *build.FILE_FLAGS.get(name, []),
           "--cuda-device-only", f"-cuid={CUID}", "-c", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
    with open(out, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main(argv):
    srcs = build._sources()
    if argv:
        want = {os.path.splitext(os.path.basename(a))[0] for a in argv}
        have = {os.path.splitext(os.path.basename(s))[0] for s in srcs}
        if want - have:
            sys.exit(f"no such source in csrc/: {', '.join(sorted(want - have))}")
        srcs = [s for s in srcs if os.path.splitext(os.path.basename(s))[0] in want]
    with tempfile.TemporaryDirectory() as tmp, cf.ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        for s, h in zip(srcs, ex.map(lambda s: code_object_hash(s, tmp), srcs)):
            print(f"{os.path.splitext(os.path.basename(s))[0]}  {h[:16]}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
