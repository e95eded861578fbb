"""Device-code comparison of two builds of the library, object by object (no GPU, no recompilation):

    python tools/isa_diff.py PARENT_BUILD_DIR NEW_BUILD_DIR [more PARENT NEW pairs] > profiles/NAME_isa_diff.txt

The proof a refactor of otvm_amd/csrc/ owes: build the parent commit and the new tree with the same compiler and build.py (the
shipping objects in csrc/build, the -DOTVM_PROBES ones in csrc/build_probes), then compare.  For every object the gfx950 code object
is unbundled as tools/isa_audit.py does; the sets of kernel symbols must be equal, and every function's disassembly must be equal
once the address column is removed.  A function whose instruction TEXT is equal but whose encodings differ only moved relative to
another symbol (a PC-relative offset): it is counted as equal and listed.  For a function that differs, the resource rows (VGPR,
AGPR, SGPR, LDS, scratch) of both sides are printed.  Exit status 1 if anything differs."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_audit import code_objects, functions, resources   # noqa: E402


def normalised(body):
    """(instruction text + encoding, instruction text alone) per line: '\\tv_add ...  // 0000000012A4: 7E000280' without the address"""
    full, text = [], []
    for line in body:
        m = re.match(r"^(.*?)\s*//\s*[0-9A-Fa-f]+:\s*(.*)$", line)
        ins, enc = (m.group(1).strip(), m.group(2).strip()) if m else (line.strip(), "")
        full.append(ins + " | " + enc)
        text.append(ins)
    return full, text


def load(build):
    out = {}
    for o, notes, dis in code_objects(build):
        out[o] = (functions(dis), {r[0]: r[1:] for r in resources(notes, dis)})
    return out


def compare(parent_dir, new_dir):
    print("## %s  vs  %s" % (parent_dir, new_dir))
    parent, new = load(parent_dir), load(new_dir)
    bad = 0
    if sorted(parent) != sorted(new):
        print("OBJECTS DIFFER: only parent %s, only new %s" % (sorted(set(parent) - set(new)), sorted(set(new) - set(parent))))
        bad += 1
    tot_k = tot_f = tot_diff = tot_moved = tot_ins = 0
    for o in sorted(set(parent) & set(new)):
        (pf, pr), (nf, nr) = parent[o], new[o]
        if sorted(pr) != sorted(nr) or sorted(pf) != sorted(nf):
            bad += 1
            print("%-24s SYMBOLS DIFFER: only parent %s, only new %s" % (o, sorted((set(pr) | set(pf)) - (set(nr) | set(nf))),
                                                                         sorted((set(nr) | set(nf)) - (set(pr) | set(pf)))))
        differ, moved = [], []
        for name in sorted(set(pf) & set(nf)):
            a, b = normalised(pf[name]), normalised(nf[name])
            if a[0] != b[0]:
                (moved if a[1] == b[1] else differ).append(name)
        print("%-24s kernels %4d  functions compared %4d  differ %d  equal up to a PC-relative offset %d" %
              (o, len(set(pr) & set(nr)), len(set(pf) & set(nf)), len(differ), len(moved)))
        for name in moved:
            print("    moved only: %s" % name)
        for name in differ:
            print("    DIFFERS: %s (%d vs %d instructions)" % (name, len(pf[name]), len(nf[name])))
            print("        VGPR AGPR SGPR LDS scratch spilled scratch-instructions: parent %s  new %s" % (pr.get(name), nr.get(name)))
        tot_k += len(set(pr) & set(nr))
        tot_f += len(set(pf) & set(nf))
        tot_ins += sum(len(pf[n]) for n in set(pf) & set(nf))
        tot_diff += len(differ)
        tot_moved += len(moved)
        if pr != nr:
            bad += 1
            for name in sorted(set(pr) & set(nr)):
                if pr[name] != nr[name]:
                    print("    RESOURCES DIFFER: %s parent %s new %s" % (name, pr[name], nr[name]))
    print("# total: %d objects, %d kernels, %d functions (%d instructions on the parent's side) compared, %d differ, "
          "%d equal up to a PC-relative offset\n" % (len(set(parent) & set(new)), tot_k, tot_f, tot_ins, tot_diff, tot_moved))
    return bad + tot_diff


def main():
    dirs = sys.argv[1:]
    if not dirs or len(dirs) % 2:
        sys.exit(__doc__)
    print("# tools/isa_diff.py: gfx950 code objects of two builds, function by function (address column removed)")
    return 1 if sum(compare(dirs[i], dirs[i + 1]) for i in range(0, len(dirs), 2)) else 0


if __name__ == "__main__":
    sys.exit(main())
