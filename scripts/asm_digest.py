"""SHA-256 of the release device assembly of every ncnet_amd/csrc/*.hip.

Run from the root of a tree (so only relative paths reach the compiler):

    python scripts/asm_digest.py OUTDIR [-j N]

Each source is compiled with build.py's HIP_FLAGS plus ``--cuda-device-only
-S -cuid=0``; comment-only lines and the directives that carry a file name or a
compiler version (``.file``, ``.ident``) are dropped, the rest is written to
OUTDIR/<stem>.s and hashed.  Prints a markdown table ``file | sha256``.  Two
trees whose tables agree run the same instructions with the same kernel
descriptors (.amdhsa_* and the metadata note are part of the hashed text).
"""
import concurrent.futures as cf
import hashlib
import importlib.util
import subprocess
import sys
from pathlib import Path


def main():
    out = Path(sys.argv[1])
    jobs = int(sys.argv[sys.argv.index("-j") + 1]) if "-j" in sys.argv else 8
    out.mkdir(parents=True, exist_ok=True)
    spec = importlib.util.spec_from_file_location("ncnet_build", "ncnet_amd/build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)

    def one(src):
        rel = Path("ncnet_amd/csrc") / src.name
        raw = out / (src.stem + ".raw.s")
        # -cuid: the __hip_cuid_<hash> marker symbol is otherwise a hash of the source text
        subprocess.run([b.HIPCC, *b.HIP_FLAGS, "-I", "ncnet_amd/csrc", "--cuda-device-only", "-S", "-cuid=0", str(rel),
                        "-o", str(raw)], check=True)
        keep = [ln.rstrip() for ln in raw.read_text().splitlines()
                if ln.strip() and not ln.lstrip().startswith((";", "//", ".file", ".ident"))]
        text = "\n".join(keep) + "\n"
        (out / (src.stem + ".s")).write_text(text)
        raw.unlink()
        return src.name, hashlib.sha256(text.encode()).hexdigest()

    with cf.ThreadPoolExecutor(jobs) as ex:
        rows = list(ex.map(one, sorted(Path("ncnet_amd/csrc").glob("*.hip"))))
    print("| file | sha256 of the stripped device assembly |\n|---|---|")
    for name, h in rows:
        print(f"| {name} | {h} |")


if __name__ == "__main__":
    main()
