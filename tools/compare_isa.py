"""Two ISA texts of one source, kernel by kernel (developer aid; profiles/sweep_forms_ab.txt).

Compile the parent's and the candidate's source as tools/count_isa.py's docstring shows (the build's flags,
--cuda-device-only -S; for a plugin build add -DOBE_PLUGIN_MODEL_HEADER='"<generated header>"'), then

    python tools/compare_isa.py parent.s candidate.s

prints whether both hold the same kernels, how many are identical line for line (local labels and the loop comments that name them, which carry
the function's position in the file, are made anonymous first), and for every kernel that differs its registers, scratch,
LDS and instruction count on both sides; then the instantiations and instruction lines per kernel name."""
import re
import subprocess
import sys

STATS = r"; (NumSgprs|NumVgprs|NumAgprs|ScratchSize|LDSByteSize|Occupancy|SGPRSpill\S*|VGPRSpill\S*):? *(\d+)"


def kernels(path):
    text = open(path).read()
    for pattern, anonymous in ((r"\.LBB\d+_", ".LBB_"), (r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1"), (r"\.LJTI\d+_", ".LJTI_"),
                               (r"\.Ltmp\d+", ".Ltmp"), (r"(Header=|Loop )BB\d+_", r"\1BB_")):
        text = re.sub(pattern, anonymous, text)
    lines = text.split("\n")
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)}
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M):
        s = e = start[name]
        while not lines[e].startswith(".Lfunc_end"):
            e += 1
        stats = {}
        for l in lines[e:e + 80]:
            if l.startswith("\t.section"):
                break
            m = re.match(STATS, l.strip())
            if m:
                stats[m.group(1)] = int(m.group(2))
        stats["instructions"] = sum(1 for l in lines[s:e] if l.startswith("\t") and not l.strip().startswith((";", ".")))
        out[name] = (lines[s:e], stats)
    return out


def main(parent, candidate):
    a, b = kernels(parent), kernels(candidate)
    names = sorted(set(a) | set(b))
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    plain = dict(zip(names, plain))
    short = lambda n: re.sub(r"^void |obe::|[<(].*", "", plain[n])
    print(f"{len(a)} kernels in the parent, {len(b)} in the candidate; the same names: {set(a) == set(b)}")
    for n in sorted(set(a) ^ set(b)):
        print("  only in the", "parent:" if n in a else "candidate:", plain[n][:160])
    both = [n for n in names if n in a and n in b]
    differ = [n for n in both if a[n][0] != b[n][0]]
    print(f"identical line for line: {len(both) - len(differ)} of {len(both)}; "
          f"registers, scratch, LDS or instruction count differ: {sum(a[n][1] != b[n][1] for n in both)}")
    print(f"instruction lines in all: {sum(s['instructions'] for _, s in a.values())} -> "
          f"{sum(s['instructions'] for _, s in b.values())}")
    for n in differ:
        print(f"  differs: {plain[n][:160]}\n    parent    {a[n][1]}\n    candidate {b[n][1]}")
    per = {}
    for n in b:
        per.setdefault(short(n), []).append(b[n][1]["instructions"])
    for k, v in sorted(per.items()):
        print(f"  {k:28s} {len(v):3d} instantiations {sum(v):7d} instruction lines")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
