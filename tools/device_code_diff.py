#!/usr/bin/env python3
"""Show that a change to csrc/ left the compiled device code alone.

    tools/device_code_diff.py BASE_REV cream_amd/csrc/FILE.hip [...] [-r OLD=NEW ...]

Exports BASE_REV into a temporary directory, compiles every given file in both trees to gfx950 assembly
(device side only; flags and per-file extras from cream_amd/build.py), and compares the two builds kernel by
kernel, as a set: the code from the kernel's label through the end of its .amdhsa_kernel block, its resource
summary and its metadata entry.  -r renames symbols in the BASE text first (plain substrings, applied in the
order given: a moved namespace, a dropped template argument).  Two things differ between any two builds and
are not compared: the __hip_cuid_* lines, and the function index in local labels and the loop comments that
cite them (.LBB<i>_<n>, "Header=BB<i>_<n>": <i> counts the functions of the file in the order they are emitted).

One line per kernel; exit status 1 on any difference, missing kernel or extra kernel.  It compares two builds
and nothing else: what instructions a kernel contains is tools/isa.sh's business.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_build():
    spec = importlib.util.spec_from_file_location("_cream_build", os.path.join(ROOT, "cream_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_asm(build, tree, rel, out):
    """rel (a path below the repository root) of `tree` -> device assembly text."""
    src = os.path.join(tree, rel)
    cmd = [build._hipcc()] + build.EXTRA_FLAGS.get(os.path.basename(rel), []) + build.HIPCC_FLAGS + [
        "-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, "cream_amd", "csrc"), '-DCREAM_BUILD_TAG="diff"',
        "-x", "hip", "--cuda-device-only", "-S", src, "-o", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("compilation failed: %s\n%s" % (src, p.stdout))
    with open(out) as fh:
        return fh.read()


LOCAL_LABEL = re.compile(r"(\.L[A-Za-z_]+?|\bBB)\d+(_\d+)?\b")      # .LBB4_7, .Lfunc_end4, and "Loop: Header=BB4_7" in comments


def normalise(text, renames):
    for old, new in renames:
        text = text.replace(old, new)
    lines = [ln for ln in text.splitlines() if "__hip_cuid_" not in ln]
    return [LOCAL_LABEL.sub(lambda m: m.group(1) + (m.group(2) or ""), ln) for ln in lines]


def kernels(lines):
    """name -> {"code": [...], "res": [...], "meta": [...]} for every kernel of one assembly file."""
    out = {}
    label = {}
    for i, ln in enumerate(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):", ln)
        if m:
            label.setdefault(m.group(1), i)
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        info = next(j for j in range(end, len(lines)) if lines[j].startswith("; Kernel info:"))
        stop = next(j for j in range(info, len(lines)) if not lines[j].startswith(";"))
        res = [l for l in lines[end:info] if l.lstrip().startswith(".set " + name + ".")] + lines[info:stop]
        out[name] = {"code": lines[label[name]:end + 1], "res": res, "meta": []}
    # metadata: the YAML list under amdhsa.kernels, one entry per kernel
    if "amdhsa.kernels:" in lines:
        i = lines.index("amdhsa.kernels:") + 1
        entry = []
        while i < len(lines) and (lines[i].startswith("  ") or not lines[i].strip()):
            if lines[i].startswith("  - ") and entry:
                _file_entry(out, entry)
                entry = []
            entry.append(lines[i])
            i += 1
        if entry:
            _file_entry(out, entry)
    return out


def _file_entry(out, entry):
    for ln in entry:
        m = re.match(r"\s+\.name:\s+(\S+)", ln)
        if m and m.group(1) in out:
            out[m.group(1)]["meta"] = entry


def figures(k):
    def grab(pat, lines):
        for ln in lines:
            m = re.search(pat, ln)
            if m:
                return m.group(1)
        return "?"
    n_insn = sum(1 for ln in k["code"] if re.match(r"\s+[a-z]\w*", ln) and not ln.lstrip().startswith((".", ";")))
    return "vgpr %s agpr %s lds %s scratch %s insns %d" % (
        grab(r"; NumVgprs: (\d+)", k["res"]), grab(r"; NumAgprs: (\d+)", k["res"]),
        grab(r"\.group_segment_fixed_size:\s+(\d+)", k["meta"]), grab(r"; ScratchSize: (\d+)", k["res"]), n_insn)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("base", help="git revision to compare against")
    ap.add_argument("files", nargs="+", help="csrc/*.hip files, relative to the repository root or the current directory")
    ap.add_argument("-r", "--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in args.rename]
    rels = [os.path.relpath(os.path.abspath(f), ROOT) for f in args.files]
    build = load_build()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base")
        os.makedirs(base)
        ar = subprocess.Popen(["git", "-C", ROOT, "archive", args.base, "cream_amd/csrc", "include"], stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", base], stdin=ar.stdout)
        if ar.wait() != 0:
            sys.exit("git archive %s failed" % args.base)
        with ThreadPoolExecutor(max_workers=2 * len(rels)) as ex:
            jobs = {(side, rel): ex.submit(compile_asm, build, tree, rel, os.path.join(tmp, "%s_%d.s" % (side, i)))
                    for i, rel in enumerate(rels) for side, tree in (("base", base), ("new", ROOT))}
            for rel in rels:
                old = kernels(normalise(jobs[("base", rel)].result(), renames))
                new = kernels(normalise(jobs[("new", rel)].result(), []))
                print("%s: %d kernels at %s, %d now" % (rel, len(old), args.base, len(new)))
                for name in sorted(set(old) | set(new)):
                    if name not in new:
                        print("  MISSING    %s" % name)
                    elif name not in old:
                        print("  EXTRA      %s" % name)
                    elif old[name] == new[name]:
                        print("  identical  %s" % name)
                        continue
                    else:
                        parts = [p for p in ("code", "res", "meta") if old[name][p] != new[name][p]]
                        print("  DIFFERENT  %s (%s)\n      base: %s\n      new:  %s" % (name, ", ".join(parts), figures(old[name]), figures(new[name])))
                    bad += 1
    print("device code: %s" % ("%d kernel(s) differ" % bad if bad else "identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
