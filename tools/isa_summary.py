"""Per-function summary of a gfx950 assembly file, and the comparison of two.

  hipcc <the Makefile's flags> --cuda-device-only -S -o a.s csrc/hz_env.hip
  python tools/isa_summary.py a.s            # one table
  python tools/isa_summary.py a.s b.s        # a -> b, function by function

For every function: the instruction count, the mnemonic histogram (as its
number of distinct mnemonics and a digest), a digest of the instruction text
with the block labels' function numbers taken out (they follow the order of
the functions in the file, not their code), and the resource lines the
compiler prints after each kernel (SGPR, VGPR, AGPR, LDS, scratch,
occupancy).  The comparison prints a markdown table and says, per function,
whether the text is identical, or else whether count and histogram are."""
import collections
import hashlib
import re
import sys

BEGIN = re.compile(r"^(\S+):\s+; @")
END = re.compile(r"^\.Lfunc_end\d+:")
INSTR = re.compile(r"^\t([a-z][a-z0-9_]*)\b")
LABEL = re.compile(r"\.LBB\d+_")
INFO = {"TotalNumSgprs": "sgpr", "NumVgprs": "vgpr", "NumAgprs": "agpr", "ScratchSize": "scratch",
        "LDSByteSize": "lds", "Occupancy": "occupancy"}
INFO_LINE = re.compile(r"^; (\w+)\s*:\s*(\d+)")


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()[:12]


def summarize(path):
    out = collections.OrderedDict()
    name, lines, last = None, [], None
    for line in open(path):
        m = BEGIN.match(line)
        if m:
            name, lines = m.group(1), []
            continue
        if name and END.match(line):
            hist = collections.Counter(INSTR.match(x).group(1) for x in lines)
            out[name] = last = {
                "instructions": len(lines), "mnemonics": len(hist),
                "histogram": digest(repr(sorted(hist.items()))),
                "text": digest("".join(LABEL.sub(".LBB_", x) for x in lines))}
            name = None
            continue
        if name:
            if INSTR.match(line):
                lines.append(line.split(";")[0].rstrip() + "\n")
        elif last is not None:
            m = INFO_LINE.match(line)
            if m and m.group(1) in INFO:
                last.setdefault(INFO[m.group(1)], int(m.group(2)))
    return out


def short(name):
    """The function's own identifier out of its mangled name (the last of the
    leading <length><identifier> run), with two bool template arguments."""
    if not name.startswith("_Z"):
        return name
    p, base = 3 if name[2:3] == "N" else 2, name
    while True:
        m = re.compile(r"\d+").match(name, p)
        if not m:
            break
        base = name[m.end():m.end() + int(m.group())]
        p = m.end() + int(m.group())
    t = re.match(r"ILb(\d)ELb(\d)E", name[p:])
    return base + (f"<{t.group(1)},{t.group(2)}>" if t else "")


RES = ("sgpr", "vgpr", "agpr", "lds", "scratch", "occupancy")


def main(argv):
    a = summarize(argv[1])
    if len(argv) == 2:
        print("| function | instructions | mnemonics | " + " | ".join(RES) + " |")
        print("|---|---|---|" + "---|" * len(RES))
        for k, v in a.items():
            print(f"| `{short(k)}` | {v['instructions']} | {v['mnemonics']} | "
                  + " | ".join(str(v.get(r, "")) for r in RES) + " |")
        return 0
    b = summarize(argv[2])
    print("| function | instructions | " + " | ".join(RES) + " | code |")
    print("|---|---|" + "---|" * len(RES) + "---|")
    for k in list(a) + [k for k in b if k not in a]:
        x, y = a.get(k), b.get(k)
        if x is None or y is None:
            print(f"| `{short(k)}` | {'only in the ' + ('first' if y is None else 'second')} |" + " |" * (len(RES) + 1))
            continue
        same = "identical text" if x["text"] == y["text"] else (
            "same count and histogram" if (x["instructions"], x["histogram"]) == (y["instructions"], y["histogram"])
            else "differs")
        cells = [f"{x.get(r, '')} -> {y.get(r, '')}" if x.get(r) != y.get(r) else str(x.get(r, "")) for r in RES]
        n = f"{x['instructions']} -> {y['instructions']}" if x["instructions"] != y["instructions"] else str(x["instructions"])
        print(f"| `{short(k)}` | {n} | " + " | ".join(cells) + f" | {same} |")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
