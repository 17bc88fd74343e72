"""Is the device code of two trees the same?  The gate of a refactor that moves kernels and helpers between files.
  python tools/isa_same.py PARENT_DIR BRANCH_DIR
Each directory holds the device assembly of every csrc/*.hip of one tree, one .s per source, compiled with the flags of
build_native.py (FLAGS + that file's SOURCE_FLAGS [+ -DMAGAT_DEBUG_HOOKS]) plus `-S --cuda-device-only`.  Functions (label
`_Z...:` to `.Lfunc_end`, which takes in a kernel's .amdhsa_* block) and the kernels' .amdgpu_metadata entries are keyed by
mangled name and compared ACROSS files: a kernel may have moved.  Normalised away: the function index in local labels,
comments (whole lines, and the "; in Loop: Header=BB<n>_<m>" kind behind a label) and .file / .loc / .ident lines.  Not compared: the __hip_cuid_<hash of the path> lines and the order of
functions.  Prints one line per differing function and exits non-zero if there is any."""
import glob
import os
import re
import sys

LABEL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)(\d+)")
BEGIN = re.compile(r"^(_Z\w+):")
DROP = re.compile(r"^\s*(;|\.file\b|\.loc\b|\.ident\b|$)")


def norm(line):
    return LABEL.sub(lambda m: "." + m.group(1) + "#", line.split(";")[0].rstrip())


def read_tree(d):
    """-> ({name: [(file, lines)]}, {name: [(file, lines)]}): functions and metadata entries, every definition found"""
    funcs, meta = {}, {}
    files = sorted(glob.glob(os.path.join(d, "*.s")))
    if not files:
        sys.exit("no .s files in " + d)
    for path in files:
        f = os.path.basename(path)
        name, body, in_meta, entry = None, [], False, []
        for line in open(path):
            if in_meta:
                if not line.startswith("    "):     # the next kernel's entry ("  - ") or the end of the list
                    if entry:
                        nm = [l.split()[-1] for l in entry if l.strip().startswith(".name:")][0]
                        meta.setdefault(nm, []).append((f, entry))
                    entry = []
                    in_meta = line.startswith("  - ")
                if in_meta:
                    entry.append(line.rstrip())
                continue
            if line.startswith("amdhsa.kernels:"):
                in_meta = True
                continue
            m = BEGIN.match(line)
            if m and name is None:
                name, body = m.group(1), []
            elif name is not None and line.startswith(".Lfunc_end"):
                funcs.setdefault(name, []).append((f, body))
                name = None
            elif name is not None and not DROP.match(line):
                body.append(norm(line))
    return funcs, meta


def first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "line %d: %r != %r" % (i, x.strip(), y.strip())
    return "length %d != %d" % (len(a), len(b))


def main(parent, branch):
    bad = 0
    (pf, pm), (bf, bm) = read_tree(parent), read_tree(branch)
    for what, p, b in (("function", pf, bf), ("metadata", pm, bm)):
        for nm in sorted(set(p) | set(b)):
            pd, bd = p.get(nm, []), b.get(nm, [])
            if len(pd) != 1 or len(bd) != 1:
                print("%s %s: defined %d x in the parent %s, %d x in the branch %s" % (what, nm, len(pd), [f for f, _ in pd], len(bd), [f for f, _ in bd]))
                bad += 1
            elif pd[0][1] != bd[0][1]:
                print("%s %s (%s -> %s): %s" % (what, nm, pd[0][0], bd[0][0], first_diff(pd[0][1], bd[0][1])))
                bad += 1
    moved = sum(1 for nm in pf if nm in bf and len(pf[nm]) == 1 and len(bf[nm]) == 1 and pf[nm][0][0] != bf[nm][0][0])
    print("%d functions (%d kernels) in the parent, %d (%d) in the branch, %d in another file, %d differ" % (len(pf), len(pm), len(bf), len(bm), moved, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
