#!/usr/bin/env python3
"""Compares the gfx950 instruction streams of kernels between two sets of device assembly files (hipcc -S --cuda-device-only).

    python tools/compare_kernel_isa.py old.s -- new1.s new2.s ...

Used when volume.hip was split into one translation unit per kernel family (round 5): every kernel of the old file must come out
of its new file instruction for instruction.  Function names are compared with the anonymous-namespace and namespace qualifiers
removed (shared types moved from an anonymous namespace to `opv`); labels, comments and directives are dropped, branch targets are
replaced by their distance in instructions.

A kernel template that has gained ONE trailing template parameter (k_integrate's SIGNED) is matched too: an old instantiation without
a namesake in the new files is compared with the new one that carries its arguments plus one more, the false / zero one where several
do (the parameter's default); so is a kernel that was no template and has become one with a single parameter (k_prepare_frames' KAFAST).
Of a kernel that differs the differing lines are printed, and whether they differ in immediate operands
only (an explicit kernel argument more moves the implicit ones behind it).  Every kernel is listed with the registers and the scratch
its metadata states: (VGPRs, SGPRs, scratch bytes)."""
import difflib
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", s):
                body.append(("label", s[:-1]))
            continue
        body.append(("inst", s))
    return out


def resources(path):
    """mangled name -> (vgpr_count, sgpr_count, private_segment_fixed_size) of the file's kernel metadata"""
    out, cur = {}, {}
    for line in open(path):
        m = re.match(r"^\s+(?:- )?\.(name|vgpr_count|sgpr_count|private_segment_fixed_size):\s+(\S+)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if len(cur) == 4:  # (the four keys of one kernel's entry, in the alphabetical order the compiler writes them)
            out[cur["name"]] = (int(cur["vgpr_count"]), int(cur["sgpr_count"]), int(cur["private_segment_fixed_size"]))
            cur = {}
    return out


def normalise(body):
    labels, n = {}, 0
    for kind, s in body:
        if kind == "label":
            labels[s] = n
        else:
            n += 1
    res, i = [], 0
    for kind, s in body:
        if kind != "inst":
            continue
        s = re.sub(r"\.LBB\d+_\d+", lambda m: "L%+d" % (labels.get(m.group(0), 0) - i), s)
        res.append(s)
        i += 1
    return res


def key(mangled):
    # drop namespace qualifiers of the function and of its parameter types: compare by kernel name + template arguments
    k = re.search(r"\d+(k_[a-z_]+)", mangled).group(1)
    t = re.search(r"\d+k_[a-z_]+(I(?:L[bij][0-9]+E)+E)?", mangled).group(1) or ""
    return k + t


def load(paths):
    out = {}
    for p in paths:
        res = resources(p)
        for n, b in kernels(p).items():
            out[key(n)] = (p.split("/")[-1], normalise(b), res.get(n))
    return out


def one_more_argument(k, new):
    """the new kernel that carries k's template arguments and one more (its default: false / zero where there is a choice)"""
    if not re.search(r"I(?:L[bij][0-9]+E)+E$", k):
        # no mangled template-argument group behind the name (key() appends it): a kernel that was no template and has become one with a
        # single parameter (k_prepare_frames' KAFAST)
        c = sorted(n for n in new if re.fullmatch(re.escape(k) + r"IL[bij][0-9]+EE", n))
    else:
        c = sorted(n for n in new if re.fullmatch(re.escape(k[:-1]) + r"L[bij][0-9]+EE", n))
    zero = [n for n in c if re.search(r"L[bij]0EE$", n)]
    return (zero or c or [None])[0]


def immediates(s):
    return re.sub(r"(?<![\w.])(?:0x[0-9a-f]+|\d+)\b", "#", s)


def main():
    sep = sys.argv.index("--")
    old, new = load(sys.argv[1:sep]), load(sys.argv[sep + 1:])
    bad, matched = 0, set()
    for k in sorted(old):
        _p0, b0, r0 = old[k]
        k1 = k if k in new else one_more_argument(k, new)
        if k1 is None:
            print("%-44s MISSING in the new files, was %s" % (k, r0)); bad += 1; continue
        matched.add(k1)
        p, b, r = new[k1]
        same = b == b0
        imm = not same and len(b) == len(b0) and all(immediates(x) == immediates(y) for x, y in zip(b0, b))
        verdict = "identical" if same else "identical but for immediates" if imm else "DIFFERENT (%d)" % len(b)
        print("%-44s %6d instructions  %s  %s  (%s%s)" % (k, len(b0), verdict, r, p, "" if k1 == k else " as " + k1))
        if not same:
            for d in difflib.unified_diff(b0, b, "old", "new", n=0, lineterm=""):
                if not d.startswith(("---", "+++")):
                    print("    " + d)
        bad += not (same or imm)
    for k in sorted(set(new) - matched):
        print("%-44s only in the new files  %s  (%s)" % (k, new[k][2], new[k][0]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
