#!/usr/bin/env python3
"""Does a source change alter the device code?  Needs hipcc, no GPU.

    scripts/device_asm_diff.py <old tree> <new tree> [--cache DIR] [--only GLOB]

For every csrc/*.hip of the two trees (say the parent commit in a `git worktree` and the working tree) and every flag set
build.py can produce for it (default, --mpr, --experimental: FLAGS and variant_flags() of each tree's own build.py), the
translation unit is compiled to gfx950 assembly (--cuda-device-only -S) and compared PER SYMBOL: the instruction text of every
kernel and every out-of-line device function, its .amdhsa_* block, the resource comments behind it (registers, LDS, scratch,
spills, occupancy) and its entry in the .amdgpu_metadata note.  Allowed to differ: the __hip_cuid_<hash> object (derived from the
file's path), the order in which symbols appear, and the numbers of assembler-local labels (.LBB<function>_<block>, .Ltmp<n>:
they count functions in order of appearance).  One line per translation unit and flag set (and one for
a translation unit that only one tree has); exit status 1 on any other difference.

--cache DIR keeps the assembly keyed by a hash of the tree's sources, the flags and the file: the old tree is then compiled once.
tu_tree.hip alone takes minutes per flag set, which is why this is a script and not a test.
"""
from __future__ import annotations

import argparse
import fnmatch
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

VARIANTS = [("default", {}), ("mpr", {"mpr": True}), ("experimental", {"exp": True})]
SLOW_FIRST = ("tu_tree", "tu_narrow", "tu_chain", "tu_pipe")


def load_build(tree):
    spec = importlib.util.spec_from_file_location("build_" + hashlib.md5(tree.encode()).hexdigest(), os.path.join(tree, "so101_sim_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(build, src, flags, cache):
    key = None
    if cache:
        h = hashlib.sha256(" ".join(flags).encode() + os.path.basename(src).encode())
        for p in build.sources():
            h.update(os.path.basename(p).encode())
            h.update(open(p, "rb").read())
        key = os.path.join(cache, h.hexdigest()[:24] + ".s")
        if os.path.exists(key):
            return open(key).read()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.s")
        subprocess.check_call([build.HIPCC, *flags, "--cuda-device-only", "-S", "-o", out, src])
        text = open(out).read()
    if key:
        os.makedirs(cache, exist_ok=True)
        with open(key + ".tmp%d" % os.getpid(), "w") as f:
            f.write(text)
        os.replace(f.name, key)
    return text


_START = re.compile(r"^\s*\.type\s+([^,\s]+),@(function|object)")
_LEAD = re.compile(r"^\s*\.(globl|protected|weak|hidden|p2align|text|section|local|comm)\b")
_LOCAL = re.compile(r"\.L[A-Za-z_]+\d+|\bBB\d+(?=_\d)")          # (BB<function>_<block>: the same labels in the loop comments)


def symbols(text):
    """{symbol: normalised text}: one chunk per function / object (from its .globl/.type lines to the next symbol's), one per
    kernel entry of the metadata note, and the file's preamble."""
    body, _, rest = text.partition("\t.amdgpu_metadata")
    note, _, tail = rest.partition("\t.end_amdgpu_metadata")
    chunks, name, cur = {}, "<preamble>", []
    for line in body.splitlines() + tail.splitlines():
        m = _START.match(line)
        if m:
            lead = []
            while cur and (_LEAD.match(cur[-1]) or not cur[-1].strip()):
                lead.insert(0, cur.pop())
            chunks[name] = cur
            name, cur = m.group(1), lead
        cur.append(line)
    chunks[name] = cur
    # (the file's epilogue - padding and the register maximums - follows whichever symbol comes last: a chunk of its own)
    for name, lines in list(chunks.items()):
        k = next((i for i, l in enumerate(lines) if ".AMDGPU.gpr_maximums" in l), None)
        if k is not None:
            while k > 0 and re.match(r"\s*\.(text|p2alignl|fill)\b", lines[k - 1]):
                k -= 1
            chunks[name], chunks["<epilogue>"] = lines[:k], lines[k:]
    out = {}
    for name, lines in chunks.items():
        if name.startswith("__hip_cuid_"):
            continue
        ids = {}
        # (the comment behind a label is aligned to the label's length, which changes with the function's number)
        norm = [re.sub(r"\s+;", " ;", _LOCAL.sub(lambda m: ids.setdefault(m.group(0), ".L%d" % len(ids)), l)) for l in lines if l.strip() and "__hip_cuid_" not in l]
        out[name] = "\n".join(norm)
    entry = []
    for line in note.splitlines() + ["  - end"]:
        if (line.startswith("  - ") or line.startswith("amdhsa.")) and entry:          # (amdhsa.target / amdhsa.version close the note, behind the last kernel)
            m = re.search(r"^\s+\.name:\s+(\S+)", "\n".join(entry), re.M)
            out["<metadata> " + (m.group(1) if m else entry[0])] = "\n".join(entry)
            entry = []
        entry.append(line)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--cache", help="directory that keeps compiled assembly between runs")
    ap.add_argument("--only", default="*", help="glob over translation-unit file names (default: all)")
    ap.add_argument("--variants", default=",".join(v for v, _ in VARIANTS), help="comma-separated subset of: " + ", ".join(v for v, _ in VARIANTS))
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1), help="compile jobs (at most 16)")
    a = ap.parse_args()
    trees = [os.path.abspath(a.old), os.path.abspath(a.new)]
    builds = [load_build(t) for t in trees]
    names = [sorted(os.path.basename(p) for p in b.translation_units() if fnmatch.fnmatch(os.path.basename(p), a.only)) for b in builds]
    only = sorted(set(names[0]) ^ set(names[1]))          # a translation unit added or removed: reported, the others are compared
    for tu in only:
        print("%-22s only in the %s tree" % (tu, "old" if tu in names[0] else "new"), flush=True)
    jobs = [(tu, v, kw) for v, kw in VARIANTS if v in a.variants.split(",") for tu in sorted(set(names[0]) & set(names[1]))]
    jobs.sort(key=lambda j: not j[0].startswith(SLOW_FIRST))

    def one(job):
        tu, v, kw = job
        return [symbols(assembly(b, os.path.join(b.CSRC, tu), list(b.FLAGS) + b.variant_flags(**kw), a.cache)) for b in builds]

    bad = 0
    with ThreadPoolExecutor(max_workers=max(1, min(16, a.j))) as pool:
        for (tu, v, _), (old, new) in zip(jobs, pool.map(one, jobs)):
            diff = sorted(s for s in set(old) | set(new) if old.get(s) != new.get(s))
            nfun = sum(1 for s in new if not s.startswith("<"))
            if diff:
                bad += 1
                print("%-22s %-13s DIFFERENT in %d of %d symbols: %s" % (tu, v, len(diff), len(set(old) | set(new)), ", ".join(diff[:6]) + (" ..." if len(diff) > 6 else "")), flush=True)
            else:
                print("%-22s %-13s identical (%d symbols)" % (tu, v, nfun), flush=True)
    print("%d of %d compilations differ" % (bad, len(jobs)))
    return 1 if bad or only else 0


if __name__ == "__main__":
    sys.exit(main())
