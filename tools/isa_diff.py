#!/usr/bin/env python3
"""Compares two device-assembly files of the same source, kernel by kernel: python tools/isa_diff.py OLD.s NEW.s [-v]

Make the files with build_ext.FLAGS plus -DLN_ABI_HASH=... plus `--cuda-device-only -S`.  For every kernel (.amdhsa_kernel) it says
whether the instruction streams are equal once the local labels (.LBB<n>_<k>, .Lfunc_*, .Ltmp*) are renumbered in order of
appearance, and whether the kernel descriptors (.amdhsa_* lines; register, LDS and private-segment sizes of the metadata) are
equal.  Kernels that differ are listed with both instruction counts and both resource lines; -v adds a unified diff of their
streams.  Exit status 1 if anything differs."""
import difflib
import re
import sys

LABEL = re.compile(r"\.(?:LBB\d+_\d+|Lfunc_\w+|Ltmp\d+)")
META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
INFO_KEYS = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "LDSByteSize", "ScratchSize", "Occupancy")


def parse(path):
    lines = open(path).read().split("\n")
    kernels = {}
    label_at = {}
    for n, line in enumerate(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):", line)
        if m:
            label_at[m.group(1)] = n
    for n, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        name = m.group(1)
        # the function's body: from its label back up to here
        start = label_at[name]
        stream, seen = [], {}
        for raw in lines[start + 1:n]:
            text = raw.split(";", 1)[0].strip()
            if not text or (text.startswith(".") and not LABEL.match(text)):
                continue  # comments, directives
            stream.append(LABEL.sub(lambda l: seen.setdefault(l.group(0), ".L%d" % len(seen)), text))
        end = next(k for k in range(n, len(lines)) if ".end_amdhsa_kernel" in lines[k])
        desc = [l.strip() for l in lines[n + 1:end]]
        info = {}
        for raw in lines[end:]:
            if raw.startswith("\t.protected") or raw.startswith("\t.amdgpu_metadata"):
                break
            m2 = re.match(r";\s*(\w+)\s*:\s*(\d+)", raw)
            if m2 and m2.group(1) in INFO_KEYS:
                info.setdefault(m2.group(1), int(m2.group(2)))
        kernels[name] = {"stream": stream, "desc": desc, "info": info, "meta": {}}
    text = "\n".join(lines)
    if "amdhsa.kernels:" in text:
        meta = text.split("amdhsa.kernels:", 1)[1].split("\namdhsa.", 1)[0]
        for entry in re.split(r"\n  - ", meta):
            m = re.search(r"\.name:\s+(\S+)", entry)
            if m and m.group(1) in kernels:
                kernels[m.group(1)]["meta"] = {k: int(v) for k, v in re.findall(r"\.(%s):\s+(\d+)" % "|".join(META_KEYS), entry)}
    return kernels


def instructions(stream):
    return sum(1 for s in stream if not s.endswith(":"))


def resources(k):
    return " ".join("%s=%s" % (key, k["info"].get(key, "?")) for key in INFO_KEYS)


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = parse(args[0]), parse(args[1])
    equal = code_diff = desc_diff = 0
    for name in sorted(set(old) & set(new)):
        a, b = old[name], new[name]
        same_code = a["stream"] == b["stream"]
        same_desc = a["desc"] == b["desc"] and a["meta"] == b["meta"]
        if same_code and same_desc:
            equal += 1
            continue
        code_diff += not same_code
        desc_diff += not same_desc
        print("DIFFERS %s: instructions %s, descriptor %s" % (name, "equal" if same_code else "differ", "equal" if same_desc else "differ"))
        print("    old: %d instructions  %s" % (instructions(a["stream"]), resources(a)))
        print("    new: %d instructions  %s" % (instructions(b["stream"]), resources(b)))
        if verbose and not same_code:
            for d in difflib.unified_diff(a["stream"], b["stream"], "old", "new", lineterm="", n=2):
                print("      " + d)
    for name in sorted(set(old) - set(new)):
        print("ONLY IN OLD %s: %d instructions  %s" % (name, instructions(old[name]["stream"]), resources(old[name])))
    for name in sorted(set(new) - set(old)):
        print("ONLY IN NEW %s: %d instructions  %s" % (name, instructions(new[name]["stream"]), resources(new[name])))
    print("%d kernels in old, %d in new, %d in both: %d equal, %d differ in instructions, %d differ in descriptor; %d only in old, %d only in new"
          % (len(old), len(new), len(set(old) & set(new)), equal, code_diff, desc_diff, len(set(old) - set(new)), len(set(new) - set(old))))
    return 0 if equal == len(old) == len(new) else 1


if __name__ == "__main__":
    sys.exit(main())
