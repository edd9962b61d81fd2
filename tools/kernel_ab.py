#!/usr/bin/env python3
"""Are the kernels of this tree the kernels of another tree?  Device assembly of the kernel translation units, one tree against the
other, as the library builds them (hipcc --cuda-device-only -S with build.py's flags of THIS tree; no GPU needed).  The check of a
refactor that must not change a kernel.
usage: kernel_ab.py PARENT_TREE [unit ...]   (PARENT_TREE: a checkout of the commit to compare against, e.g. a `git worktree` outside
the repository; default units: every .hip of this tree's build.SOURCES.  At most 8 compiles run at a time.)
Prints one line per unit: kernels (.amdhsa_kernel entries) parent / tree, names on one side only, kernels whose next_free_vgpr /
next_free_sgpr / group_segment_fixed_size / private_segment_fixed_size or instruction count differ, kernels whose body text differs
(comments dropped; of a local label the function's index is dropped, the block's number kept), instructions parent / tree; then a
total.  Device functions that are no kernels are compared in the same way where both sides have them and listed where one side
has them (an include that went away takes its out-of-line functions with it: that is no difference of a kernel).
Exit status 1 if a kernel differs or exists on one side only or a device function that both sides have differs, 2 if a unit
does not compile.
It reads the structure of the assembly only: symbols, the kernel descriptors, the text between a symbol and its end.
profiles/r12_kernel_headers_ab.txt is its output."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from datafusion_archive_amd import build as B  # noqa: E402
from tools.kernel_meta import demangle  # noqa: E402

FIGURES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def functions(asm):
    """{symbol: (is_kernel, figures, instruction count, normalised body)} of one unit's device assembly"""
    out = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        name, text = m.group(1), m.group(2)
        desc = re.search(r"^\t\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)^\t\.end_amdhsa_kernel", text, re.S | re.M)
        figures = tuple(int(re.search(r"\.amdhsa_" + k + r" (\d+)", desc.group(1)).group(1)) for k in FIGURES) if desc else ()
        lines = [ln.split(";")[0].rstrip() for ln in text.splitlines()]
        lines = [re.sub(r"(\.L[A-Za-z]+)\d+_", r"\1_", ln) for ln in lines if ln.strip()]
        code = text.split("\t.section\t.rodata", 1)[0] if desc else text
        n_ins = sum(1 for ln in code.splitlines() if ln.startswith("\t") and not ln.strip().startswith((".", ";")))
        out[name] = (desc is not None, figures, n_ins, "\n".join(lines))
    return out


def compile_unit(csrc, unit, out):
    src = os.path.join(csrc, unit + ".hip")
    if not os.path.exists(src):
        return {}
    flags = [f for f in B.CXXFLAGS if f != "-fPIC"]
    r = subprocess.run([B._hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, src], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{src} does not compile:\n{r.stderr[-2000:]}")
    return functions(open(out).read())


def short(names):
    pretty = demangle(sorted(names))
    return ", ".join(re.sub(r"\(.*", "", pretty[n]).replace("dfx::", "") for n in sorted(names))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if not args:
        sys.exit(__doc__)
    parent_csrc = os.path.join(os.path.abspath(args[0]), os.path.relpath(B.CSRC, ROOT))
    units = [u[:-4] if u.endswith(".hip") else u for u in args[1:]] or sorted(s[:-4] for s in B.SOURCES if s.endswith(".hip"))
    with tempfile.TemporaryDirectory() as td, ThreadPoolExecutor(max_workers=8) as ex:
        jobs = {(side, u): ex.submit(compile_unit, csrc, u, os.path.join(td, f"{side}_{u}.s"))
                for u in units for side, csrc in (("parent", parent_csrc), ("tree", B.CSRC))}
        total = [0, 0, 0, 0, 0]  # kernels parent / tree, instructions parent / tree, differences
        for u in units:
            try:
                a, b = jobs["parent", u].result(), jobs["tree", u].result()
            except RuntimeError as e:
                print(e)
                sys.exit(2)
            ka, kb = {n for n in a if a[n][0]}, {n for n in b if b[n][0]}
            both = ka & kb
            figures = sum(1 for n in both if a[n][1:3] != b[n][1:3])
            bodies = sum(1 for n in both if a[n][3] != b[n][3])
            ia, ib = sum(a[n][2] for n in ka), sum(b[n][2] for n in kb)
            print(f"  {u} kernels {len(ka)} / {len(kb)} only in parent {len(ka - kb)} only in tree {len(kb - ka)} figures differ {figures} "
                  f"bodies differ {bodies} instructions {ia} / {ib}", flush=True)
            fa, fb = set(a) - ka, set(b) - kb
            changed = {n for n in fa & fb if a[n][2:] != b[n][2:]}
            for what, names in (("only in parent", fa - fb), ("only in tree", fb - fa), ("differ", changed)):
                if names:
                    print(f"    device functions, no kernels, {what}: {short(names)}")
            for n in sorted(n for n in both if a[n][1:] != b[n][1:]) + sorted(ka ^ kb):
                print(f"    differs: {n}")
            total = [x + y for x, y in zip(total, (len(ka), len(kb), ia, ib, len(ka ^ kb) + len(changed) + sum(1 for n in both if a[n][1:] != b[n][1:])))]
    print(f"total kernels {total[0]} / {total[1]}, instructions {total[2]} / {total[3]}, kernels and common device functions that differ or are on one side only: {total[4]}")
    sys.exit(1 if total[4] else 0)


if __name__ == "__main__":
    main()
