"""Kernel resource tables from two compiles of one unit, side by side.

    hipcc <the Makefile's flags> -Rpass-analysis=kernel-resource-usage -c csrc/hz_mcts.hip 2> new.txt
    (the same in a checkout of the parent commit)                                            2> old.txt
    python tools/kernel_resources.py old.txt new.txt [--root-forms | --retired-knobs]

Prints, per kernel of old.txt, its SGPR / VGPR / AGPR / scratch / occupancy /
spill / LDS numbers and whether new.txt has a kernel of that name with the
same numbers, then the kernels only new.txt has.  --root-forms: new.txt's
select kernels take the root form as an int where old.txt's took the Gumbel
gate as a bool: form 0 is matched with false,
form 1 with true, and form 2 has no counterpart.  --retired-knobs: old.txt's
k_expand_backup<Waves, Sel, Root, Sym, Gather, BPW, WaveSlot> is new.txt's
<Sel, Root, Sym, Gather> where Waves is 4, BPW is Gather ? 16 : 1 and WaveSlot
is false; the other forms served knobs that are gone (DESIGN.md section 10
item 12) and are listed as retired.  Exit status 1 if a kernel of old.txt is
missing from new.txt or differs.  Cross-compiles; needs no GPU.
"""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill",
          "VGPRs Spill", "LDS Size [bytes/block]")
ROOT_ARG = {"k_select": 0, "k_select_gather_encode": 0, "k_expand_backup": 2}  # the template argument that changed


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
            return out.splitlines()
        except (OSError, subprocess.CalledProcessError):
            continue
    return list(names)


def parse(path):
    kernels, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = text.split(":", 1)[1].strip()
            kernels[cur] = {}
        elif cur is not None and ":" in text:
            key, val = text.rsplit(":", 1)
            kernels[cur][key.strip()] = val.strip()
    pretty = demangle(list(kernels))
    out = {}
    for name, nice in zip(kernels, pretty):
        nice = re.sub(r"\(anonymous namespace\)::", "", nice)
        nice = re.sub(r"^void ", "", nice)
        nice = re.sub(r"\(hz_mcts_args.*$|\(unsigned.*$|\(float.*$|\(int.*$|\(short.*$", "", nice)
        out[nice] = tuple(kernels[name].get(f, "?") for f in FIELDS)
    return out


def old_name_of(name):
    """new.txt's name of a select kernel as old.txt spelt it (None: a forced form)."""
    m = re.match(r"(\w+)<(.*)>$", name)
    if not m or m.group(1) not in ROOT_ARG:
        return name
    args = [a.strip() for a in m.group(2).split(",")]
    i = ROOT_ARG[m.group(1)]
    form = re.sub(r"^\(int\)", "", args[i])
    if form == "2":
        return None
    args[i] = {"0": "false", "1": "true"}.get(form, form)
    return f"{m.group(1)}<{', '.join(args)}>"


def knob_name_of(name):
    """old.txt's name of an expand kernel as new.txt spells it (None: a retired knob's form)."""
    m = re.match(r"k_expand_backup<(.*)>$", name)
    if not m:
        return name
    waves, sel, root, sym, gather, bpw, wave_slot = (re.sub(r"^\(\w+\)", "", a.strip()) for a in m.group(1).split(","))
    if waves != "4" or bpw != ("16" if gather == "true" else "1") or wave_slot != "false":
        return None
    return f"k_expand_backup<{sel}, {root}, {sym}, {gather}>"


def main(argv):
    root_forms = "--root-forms" in argv
    paths = [a for a in argv if not a.startswith("--")]
    old, new = parse(paths[0]), parse(paths[1])
    retired = {}
    if "--retired-knobs" in argv:
        named = {name: knob_name_of(name) for name in old}
        retired = {name: row for name, row in old.items() if named[name] is None}
        old = {named[name]: row for name, row in old.items() if named[name] is not None}
    by_old, added = {}, []
    for name, row in new.items():
        was = old_name_of(name) if root_forms else name
        if was is None or was not in old:
            added.append(name)
        else:
            by_old[was] = (name, row)
    print("| kernel | " + " | ".join(FIELDS) + " | new |")
    print("|---|" + "---|" * (len(FIELDS) + 1))
    bad = 0
    for name, row in old.items():
        got = by_old.get(name)
        verdict = "missing" if got is None else ("same" if got[1] == row else "DIFFERS " + "/".join(got[1]))
        bad += verdict != "same"
        print(f"| `{name}` | " + " | ".join(row) + f" | {verdict} |")
    for name, row in retired.items():
        print(f"| `{name}` | " + " | ".join(row) + " | retired |")
    print(f"\n{len(old) + len(retired)} kernels in {paths[0]}, {len(new)} in {paths[1]}; {len(old) - bad} with the same "
          f"numbers; {len(retired)} retired; {len(added)} new:")
    for name in added:
        print(f"  {name}: " + ", ".join(f"{f} {v}" for f, v in zip(FIELDS, new[name])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
