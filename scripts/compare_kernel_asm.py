#!/usr/bin/env python3
"""Do two source trees compile pd_kernels.hip and pd_pose.hip to the same gfx950 kernels?  (no GPU needed)

  python scripts/compare_kernel_asm.py TREE_A TREE_B [--work DIR] [--jobs N]

For each of the six rollout kernel objects of the library (segment width 16 / 32 / 64 x PD_POLICY 0 / 1) and for pd_pose (the pose and
state ops) the script takes the compile command of the tree's own Makefile (`make -n`), turns it into `-S --cuda-device-only` and
compares the two assembly files as MULTISETS of kernels:
  * the text of each kernel's body, with its own symbol name and the function index of local labels (.LBB<i>_<j>, .Lfunc_end<i>) taken
    out -- mangled names change when a template parameter goes, the instructions must not;
  * its code-object metadata: VGPR / AGPR / SGPR counts, both spill counts, static LDS, scratch size, max workgroup size.
Equal multisets: no instantiation gained or lost, none compiled differently.  Exit status 0 when all seven objects agree, 1 otherwise (the
kernels without a partner are listed by name).  Assembly is kept under --work (default: a temporary directory) and reused when neither
the sources nor the command changed, so a second run against the same baseline compiles one side only.
"""
import argparse
import collections
import concurrent.futures
import hashlib
import pathlib
import re
import shlex
import subprocess
import sys
import tempfile

OBJECTS = ["pd_kernels_16", "pd_kernels_32", "pd_kernels_64", "pd_kernels_lit_16", "pd_kernels_lit_32", "pd_kernels_lit_64", "pd_pose"]
META = [".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size", ".max_flat_workgroup_size"]


def compile_asm(tree, obj, work):
    csrc = pathlib.Path(tree) / "ppr-diffphys_amd" / "csrc"
    plan = subprocess.run(["make", "-n", "-B", f"build/{obj}.o"], cwd=csrc, check=True, capture_output=True, text=True).stdout
    cmd = next(shlex.split(ln) for ln in plan.splitlines() if f"build/{obj}.o" in ln and " -c " in ln)
    out = pathlib.Path(work) / f"{obj}.s"
    cmd = [("-S" if w == "-c" else w) for w in cmd[:cmd.index("-o")]] + ["--cuda-device-only", "-o", str(out)]
    key = hashlib.sha256()
    key.update(" ".join(cmd[:-1]).encode())
    for f in sorted(list(csrc.glob("*.h")) + list(csrc.glob("*.hip")) + [csrc / ".." / ".." / "include" / "ppr_diffphys.h"]):
        key.update(f.read_bytes())
    stamp = out.with_suffix(".key")
    if not (out.exists() and stamp.exists() and stamp.read_text() == key.hexdigest()):
        subprocess.run(cmd, cwd=csrc, check=True)
        stamp.write_text(key.hexdigest())
    return out


def kernels_of(path):
    """{kernel name: (sha256 of the normalised body, metadata tuple)}"""
    text = pathlib.Path(path).read_text()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    meta = {}
    for entry in re.split(r"^  - (?=\.)", text[text.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        f = dict(re.findall(r"^\s*(\.\w+):\s*(\S+)\s*$", entry, re.M))
        meta[f[".name"]] = tuple(f.get(k, "0") for k in META)
    out = {}
    for n in names:
        m = re.search(r"^%s:.*?^\.Lfunc_end\d+:" % re.escape(n), text, re.M | re.S)
        body = m.group(0).replace(n, "KERNEL")
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", body)
        body = re.sub(r"[ \t]*;.*$", "", body, flags=re.M)   # comments name the function index too ("in Loop: Header=BB19_38"), padded to a column
        out[n] = (hashlib.sha256(body.encode()).hexdigest(), meta[n])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--work", default=None, help="directory for the assembly files (kept and reused)")
    ap.add_argument("--jobs", type=int, default=7)
    args = ap.parse_args()
    work = pathlib.Path(args.work or tempfile.mkdtemp(prefix="kernel_asm_"))
    sides = {"a": args.tree_a, "b": args.tree_b}
    for s in sides:
        (work / s).mkdir(parents=True, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        asm = {(s, o): pool.submit(compile_asm, sides[s], o, work / s) for s in sides for o in OBJECTS}
        asm = {k: f.result() for k, f in asm.items()}
    bad = 0
    for o in OBJECTS:
        ka, kb = kernels_of(asm["a", o]), kernels_of(asm["b", o])
        ca, cb = collections.Counter(ka.values()), collections.Counter(kb.values())
        same = ca == cb
        print(f"{o}: {len(ka)} kernels / {len(kb)} kernels: {'all equal' if same else 'DIFFERENT'}")
        if not same:
            bad += 1
            for tag, ks, other in (("A only", ka, cb), ("B only", kb, ca)):
                left = collections.Counter(other)
                for n, v in sorted(ks.items()):
                    if left[v] > 0:
                        left[v] -= 1
                    else:
                        print(f"  {tag}: {n}  {dict(zip(META, v[1]))}")
    print(f"assembly kept in {work}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
