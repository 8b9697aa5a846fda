"""Per-kernel comparison of two device-side assembly listings, for changes that move kernels between files without
meaning to alter them.  Make the listings with the Makefile's flags:

    hipcc <HIPFLAGS> --cuda-device-only -S niqki_amd/csrc/FILE.hip -o FILE.s

and run  compare_kernel_isa.py before.s[,more.s] after.s[,more.s].  It matches kernels by mangled name and compares
each one's instruction text and .amdhsa_kernel descriptor after dropping comments and the function numbers of local
labels (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>).  Prints the kernel counts and "identical", or the kernels that differ or
exist on one side only; exit status 1 then.  Needs no GPU."""
import re
import sys


def kernels(paths):
    """'a.s,b.s' -> {mangled name: (instructions, descriptor)}; device functions that are no kernels are skipped."""
    out = {}
    for p in paths.split(","):
        name, body = None, []
        for line in open(p, errors="replace"):
            s = line.split(";", 1)[0].rstrip()
            if not s.strip():
                continue
            m = re.match(r"^(\w+):\s*$", s)
            if m and name is None and not s.startswith(".L"):
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            if re.match(r"^\.Lfunc_end\d+:", s):
                t = "\n".join(body)
                i, j = t.find(".amdhsa_kernel"), t.find(".end_amdhsa_kernel")
                if i >= 0:
                    out[name] = (t[:i] + t[j:], t[i:j])
                name = None
                continue
            body.append(re.sub(r"\.Ltmp\d+", ".Ltmp", re.sub(r"\.LBB\d+_", ".LBB_", s)).strip())
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    print("kernels before %d, after %d; %s" % (len(a), len(b), "identical" if not bad else bad))
    sys.exit(bool(bad))
