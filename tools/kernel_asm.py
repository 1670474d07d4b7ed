#!/usr/bin/env python3
"""Assembly text of named kernels, for proving a refactor left them untouched without a GPU.

Compiles a .hip file for the device only with the product flags of the Makefile plus `-S`,
takes each kernel whose demangled name contains one of the given substrings from its label to
its function end, drops comment-only lines, trailing comments and debug / location directives,
takes the function's ordinal out of its block labels, and prints `sha256  lines  kernel` per kernel.  With --dump DIR the stripped text is written to
DIR/<kernel>.asm too.  Also lists every non-kernel function symbol the file defines (a helper that
was meant to be inlined and is not shows up there).

usage: python3 tools/kernel_asm.py FILE.hip SUBSTR [SUBSTR ...] [--dump DIR]
"""
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wno-unused-result",
         "-Iinclude", "--cuda-device-only", "-S", "-o", "-"]
DROP = re.compile(r"^\s*(;|\.loc\b|\.file\b|\.cfi_|\.Ltmp\d+:|\.Lfunc_(begin|end)\d+:)")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return [re.sub(r"\(.*", "", o).replace("gfpl::", "").replace("void ", "") for o in out.stdout.split("\n")[:len(names)]]


def main():
    args = sys.argv[1:]
    dump = None
    if "--dump" in args:
        i = args.index("--dump")
        dump = args[i + 1]
        del args[i:i + 2]
        os.makedirs(dump, exist_ok=True)
    src, wanted = args[0], args[1:]
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + [src], cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{src}: hipcc failed\n{r.stderr[-2000:]}")
    asm = r.stdout
    lines = asm.splitlines()
    funcs = [m.group(1) for l in lines if (m := re.match(r"\s*\.type\s+(\S+),@function", l))]
    kernels = set(re.findall(r"\.amdhsa_kernel\s+(\S+)", asm))
    names = dict(zip(funcs, demangle(funcs)))
    for f in funcs:
        if f in kernels and any(w in names[f] for w in wanted):
            a = next(i for i, l in enumerate(lines) if l.startswith(f + ":"))
            b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
            body = [re.sub(r"\s*;.*$", "", l).rstrip() for l in lines[a:b] if not DROP.match(l)]
            # (block labels carry the function's ordinal in its file: .LBB<ordinal>_<block>)
            body = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in body if l]
            text = "\n".join(body) + "\n"
            print(hashlib.sha256(text.encode()).hexdigest(), len(body), names[f])
            if dump:
                with open(os.path.join(dump, re.sub(r"[^A-Za-z0-9_]+", "_", names[f]).strip("_") + ".asm"), "w") as o:
                    o.write(text)
    outofline = [names[f] for f in funcs if f not in kernels]
    print("out-of-line functions:", ", ".join(outofline) if outofline else "none")


if __name__ == "__main__":
    main()
