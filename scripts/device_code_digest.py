#!/usr/bin/env python3
"""Digest of the device code of every kernel in libsfem_hip.

For each unit of the Makefile's SRCS: compile with the Makefile's own command
line, `-c` replaced by `--offload-device-only -S`, drop the lines that name
the per-unit `__hip_cuid_<hash>` symbol, take the function's number out of the
local labels (it follows the order of instantiation), and print

    <unit> <kernel symbol> <sha256>

per kernel, where the digest covers the kernel's assembly, its
`.amdhsa_kernel` descriptor and its entry in the `.amdgpu_metadata` block.
Two trees whose outputs are equal launch the same device code; a refactor of
the host side is checked with

    python scripts/device_code_digest.py > after.txt    # and likewise before
    diff before.txt after.txt

No GPU is needed.  The output depends on the compiler, so it is not committed.
"""
import argparse
import concurrent.futures
import hashlib
import pathlib
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "swirl_fem_amd" / "csrc"
MAX_JOBS = 8
LOCAL_LABEL = re.compile(r"(\.LBB|\bBB|\.Lfunc_begin|\.Lfunc_end|\.LJTI)\d+")
COMMENT_PAD = re.compile(r"[ \t]+;")


def compile_commands(csrc):
    """{unit: argv} of the Makefile's compile lines (make -n, nothing runs)."""
    out = subprocess.run(
        ["make", "-C", str(csrc), "--no-print-directory", "-n", "-B", "all"],
        check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" in argv:
            cmds[argv[argv.index("-c") + 1]] = argv
    return cmds


def assembly(csrc, unit, argv, tmp):
    dst = pathlib.Path(tmp) / (pathlib.Path(unit).stem + ".s")
    i = argv.index("-c")
    argv = argv[:i] + ["--offload-device-only", "-S"] + argv[i + 1:]
    argv[argv.index("-o") + 1] = str(dst)
    subprocess.run(argv, check=True, cwd=csrc)
    return [normalise(l) for l in dst.read_text().splitlines()
            if "__hip_cuid_" not in l]


def normalise(line):
    """Local labels carry the function's position in the unit (.LBB12_3,
    .Lfunc_end12, `Header=BB12_9` in comments, and the column at which the
    comment starts), which moves with the order of instantiation alone."""
    return COMMENT_PAD.sub(" ;", LOCAL_LABEL.sub(r"\1", line))


def kernel_texts(lines):
    """{symbol: text}: the lines from the kernel's first directive to the next
    kernel's (or to the metadata block), plus its metadata entry."""
    names = [m.group(1) for l in lines
             if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    meta = next((n for n, l in enumerate(lines)
                 if l.strip() == ".amdgpu_metadata"), len(lines))
    starts = {}
    for n, l in enumerate(lines[:meta]):
        m = re.match(r"\s*\.(?:protected|globl|weak)\s+(\S+)", l)
        if m and m.group(1) in names and m.group(1) not in starts:
            # a template's kernel opens its own comdat section one line up
            starts[m.group(1)] = (
                n - 1 if n and lines[n - 1].lstrip().startswith(".section")
                else n)
    # the unit's trailer (register maximums, .ident) belongs to no kernel
    last = max(starts.values(), default=0)
    tail = next((n for n in range(last, meta) if lines[n].lstrip().startswith(
        ".section\t.AMDGPU.gpr_maximums")), meta)
    order = sorted(starts.values()) + [tail]
    texts = {s: lines[b:order[order.index(b) + 1]] for s, b in starts.items()}
    entries, entry = [], None
    for l in lines[meta:]:   # YAML: one "  - " item per kernel
        if l.startswith("  - "):
            entry = [l]
            entries.append(entry)
        elif entry is not None and l.startswith("    "):
            entry.append(l)
        else:
            entry = None
    for entry in entries:
        for l in entry:
            m = re.match(r"[\s-]*\.name:\s+(\S+)", l)
            if m and m.group(1) in texts:
                texts[m.group(1)] = texts[m.group(1)] + entry
    return {s: "\n".join(t) for s, t in texts.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--csrc", type=pathlib.Path, default=CSRC,
                    help="source directory with the Makefile (default: %(default)s)")
    ap.add_argument("-j", type=int, default=MAX_JOBS,
                    help="compiles at once (at most %d)" % MAX_JOBS)
    ap.add_argument("units", nargs="*", help="only these units (default: all)")
    args = ap.parse_args()
    cmds = compile_commands(args.csrc)
    units = args.units or list(cmds)
    with tempfile.TemporaryDirectory() as tmp, \
            concurrent.futures.ThreadPoolExecutor(
                max(1, min(args.j, MAX_JOBS))) as pool:
        jobs = [pool.submit(assembly, args.csrc, u, cmds[u], tmp)
                for u in units]
        kernels = 0
        for unit, job in zip(units, jobs):
            for sym, text in sorted(kernel_texts(job.result()).items()):
                print(unit, sym, hashlib.sha256(text.encode()).hexdigest())
                kernels += 1
    print("%d units, %d kernels" % (len(units), kernels), file=sys.stderr)


if __name__ == "__main__":
    main()
