#!/usr/bin/env python3
"""Compare the gfx950 machine code of the device translation units of two trees.

    scripts/kernel_isa_diff.py <before> <after> [--units goertzel fold ...]
                               [--jobs N] [--keep DIR]

<before> / <after> are each one of
  * a source tree (a directory holding audio-network_amd/csrc),
  * a git revision of this repository (extracted with `git archive` into a
    temporary directory), or
  * a directory of <unit>.s files that an earlier run left with --keep.

Every unit is compiled with its own tree's Makefile HIPFLAGS plus
`--offload-device-only -S` (CPU only; no GPU is needed). The assembly is split
into functions; each function body, together with its kernel descriptor block,
is normalised (comments stripped, every mangled symbol `_Z...` replaced by one
placeholder, the function index removed from local labels) and hashed. The two
multisets of hashes are compared per unit. Exit status 0: equal everywhere.

For every function that is not identical and has a namesake on the other side,
a second line says whether the normalised lines are equal as a multiset
("reordered": the same instructions in another order) or, failing that, whether
the mnemonics, the first token of each normalised line, are ("same
instructions, other registers or order"; else "changed"), the line count before
and after, and the kernel descriptor's register, LDS and scratch fields.

A refactor that renames or drops template parameters changes every mangled
name and nothing else; this tool proves the "nothing else". It hashes text and
looks for no particular instruction.
"""
import argparse
import collections
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

UNITS = ["goertzel", "fold", "residue", "fft_quad", "rescue", "synth", "acquire", "acquire_segments",
         "acquire_frames", "acquire_frames_segments", "frames_check", "frames_fec", "frames_rs", "frames_carry",
         "frames_tx", "frame_gpu"]
CSRC = os.path.join("audio-network_amd", "csrc")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FUNC_START = re.compile(r"^\s*\.type\s+(\S+),@function")
# what follows the last function of a unit: LDS / data objects, then metadata
TAIL_START = re.compile(r"^\s*(\.type\s+\S+,@object|\.amdgpu_metadata|\.ident|\.amdgpu_lds)\b")
MANGLED = re.compile(r"_Z[A-Za-z0-9_.$]+")
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")
DESCRIPTOR = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def compile_command(csrc):
    """`hipcc <HIPFLAGS>` as the tree's own Makefile spells it."""
    out = subprocess.run(
        ["make", "-s", "-C", csrc, "--eval", "isa-diff-flags: ; @echo $(HIPCC) $(HIPFLAGS)",
         "isa-diff-flags"], check=True, capture_output=True, text=True).stdout
    return out.split()


def compile_unit(csrc, cmd, unit, dest):
    subprocess.run(cmd + ["--offload-device-only", "-S", unit + ".hip", "-o", dest],
                   cwd=csrc, check=True)
    return unit


def normalise(line):
    if '"' not in line:
        line = line.split(";", 1)[0]
    line = MANGLED.sub("SYM", line)
    line = LOCAL_LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)
    return " ".join(line.split())


def functions(path):
    """name -> (hash, lines) of the normalised body (code + descriptor), one per function."""
    bodies, name, cur = {}, None, []
    with open(path) as f:
        for raw in f:
            m = FUNC_START.match(raw)
            if m or (name and TAIL_START.match(raw)):
                if name:
                    bodies[name] = cur
                name, cur = (m.group(1), []) if m else (None, [])
            if name:
                line = normalise(raw)
                if line:
                    cur.append(line)
    if name:
        bodies[name] = cur
    return {n: (hashlib.sha256("\n".join(b).encode()).hexdigest(), b) for n, b in bodies.items()}


def descriptor(lines):
    """The DESCRIPTOR fields of a function's .amdhsa_ block, as 'v/s/lds/scratch'."""
    got = {}
    for line in lines:
        for key in DESCRIPTOR:
            if line.startswith(".amdhsa_" + key + " "):
                got[key] = line.split()[1]
    return "/".join(got.get(key, "-") for key in DESCRIPTOR)


def mnemonics(lines):
    """The multiset of the first tokens of a function's normalised lines."""
    return collections.Counter(line.split()[0] for line in lines)


def materialise(arg, stack):
    """Directory for `arg`: (path, is_assembly)."""
    if os.path.isdir(os.path.join(arg, CSRC)):
        return arg, False
    if os.path.isdir(arg):
        return arg, True
    tmp = stack.enter_context(tempfile.TemporaryDirectory(prefix="isa_diff_tree_"))
    archive = subprocess.Popen(["git", "-C", REPO, "archive", arg, CSRC, "include"],
                               stdout=subprocess.PIPE)
    subprocess.run(["tar", "-x", "-C", tmp], stdin=archive.stdout, check=True)
    if archive.wait() != 0:
        sys.exit(f"{arg}: neither a tree, an assembly directory nor a git revision")
    return tmp, False


def main():
    import contextlib
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--units", nargs="+", default=UNITS, choices=UNITS)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly under DIR/before and DIR/after")
    args = ap.parse_args()

    with contextlib.ExitStack() as stack:
        out_root = args.keep or stack.enter_context(tempfile.TemporaryDirectory(prefix="isa_diff_"))
        asm, jobs = {}, []
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            for side, arg in (("before", args.before), ("after", args.after)):
                path, is_asm = materialise(arg, stack)
                asm[side] = path if is_asm else os.path.join(out_root, side)
                if is_asm:
                    continue
                os.makedirs(asm[side], exist_ok=True)
                csrc = os.path.join(path, CSRC)
                cmd = compile_command(csrc)
                for unit in args.units:
                    dest = os.path.abspath(os.path.join(asm[side], unit + ".s"))
                    jobs.append(pool.submit(compile_unit, csrc, cmd, unit, dest))
            for j in jobs:
                j.result()

        differ = False
        for unit in args.units:
            fa = functions(os.path.join(asm["before"], unit + ".s"))
            fb = functions(os.path.join(asm["after"], unit + ".s"))
            ca = collections.Counter(h for h, _ in fa.values())
            cb = collections.Counter(h for h, _ in fb.values())
            same = ca == cb
            differ |= not same
            print(f"{unit}: {len(fa)} functions before ({len(ca)} distinct), {len(fb)} after "
                  f"({len(cb)} distinct): {'equal' if same else 'DIFFERENT'}")
            for side, names, only in (("before", fa, ca - cb), ("after", fb, cb - ca)):
                for name, (h, _) in sorted(names.items()):
                    if h in only:
                        print(f"  only {side}: {h[:12]} {name}")
            for name in sorted(set(fa) & set(fb)):
                (ha, la), (hb, lb) = fa[name], fb[name]
                if ha != hb:
                    if collections.Counter(la) == collections.Counter(lb):
                        kind = "reordered"
                    elif mnemonics(la) == mnemonics(lb):
                        kind = "same instructions, other registers or order"
                    else:
                        kind = "changed"
                    print(f"  {kind}: {name}: lines {len(la)} -> {len(lb)}, "
                          f"vgpr/sgpr/lds/scratch {descriptor(la)} -> {descriptor(lb)}")
        print("machine code: " + ("DIFFERENT" if differ else "identical"))
        return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
