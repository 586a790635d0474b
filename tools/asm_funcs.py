#!/usr/bin/env python3
"""Are the device functions of one set of assembly files those of another?

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S -o unit.s csrc/unit.hip
    asm_funcs.py --old parent/hz_mcts.s --new hz_mcts.s hz_mcts_report.s ... [--rename NEW=OLD]

Each file is cut into functions: from the symbol's label to its .Lfunc_end,
plus its .amdhsa_kernel ... .end_amdhsa_kernel block (the descriptor: VGPRs,
SGPRs, LDS, scratch, kernarg size).  Comments go, local block labels lose
their function number, --rename replaces a substring of the new side's text
(a renamed struct's mangled name).  Prints one JSON line; exit 0 when both
sides hold the same functions with equal text (a function that several new
files hold, as a kernel defined in a shared header, must be equal in all).
"""
import argparse
import json
import re
import sys

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")


def norm(line):
    line = line.split(";", 1)[0].rstrip()
    return re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+_?", r".L\1_", line)


def functions(path, renames):
    text = open(path).read()
    for new, old in renames:
        text = text.replace(new, old)
    out, body, desc = {}, {}, {}
    name = kern = None
    for raw in text.split("\n"):
        line = norm(raw)
        m = LABEL.match(raw)
        if name is None and kern is None and m:
            name = m.group(1)
            body[name] = []
        if name is not None:
            if line:
                body[name].append(line)
            if raw.startswith(".Lfunc_end"):
                name = None
        elif raw.strip().startswith(".amdhsa_kernel "):
            kern = raw.split()[1]
            desc[kern] = [line]
        elif kern is not None:
            desc[kern].append(line.strip())
            if raw.strip() == ".end_amdhsa_kernel":
                kern = None
    for f, lines in body.items():
        if any(l.startswith(".Lfunc_end") for l in lines):  # (a data symbol has no end mark)
            out[f] = "\n".join(lines + desc.get(f, []))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--rename", action="append", default=[], metavar="NEW=OLD")
    a = ap.parse_args()
    renames = [r.split("=", 1) for r in a.rename]
    old, new, several, unequal, where = {}, {}, set(), set(), {}
    for p in a.old:
        old.update(functions(p, []))
    for p in a.new:
        for f, t in functions(p, renames).items():
            if f in new:
                several.add(f)
                if new[f] != t:
                    unequal.add(f)
            new[f] = t
            where.setdefault(p, []).append(f)
    res = {
        "old_functions": len(old),
        "new_functions": len(new),
        "per_new_file": {p: len(v) for p, v in where.items()},
        "only_old": sorted(set(old) - set(new)),
        "only_new": sorted(set(new) - set(old)),
        "in_several_new_files": sorted(several),
        "differ": sorted(unequal | {f for f in old if f in new and old[f] != new[f]}),
    }
    print(json.dumps(res))
    return 1 if res["only_old"] or res["only_new"] or res["differ"] else 0


if __name__ == "__main__":
    sys.exit(main())
