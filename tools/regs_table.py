"""Register table of a kernel source from hipcc's resource remarks: one line per kernel (demangled), VGPRs / AGPRs / spills / scratch.
usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Rpass-analysis=kernel-resource-usage -c X.hip -o /tmp/x.o 2> rem.txt
       python tools/regs_table.py rem.txt [name filter]"""
import re
import subprocess
import sys

FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("VGPRs Spill", "vspill"), ("SGPRs Spill", "sspill"),
          ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ")]


def parse(text):
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+([^:]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return rows


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return out if len(out) == len(names) else names


if __name__ == "__main__":
    rows = parse(open(sys.argv[1]).read())
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    names = demangle([r["name"] for r in rows])
    print(f"{'kernel':100s} " + " ".join(f"{h:>7s}" for _, h in FIELDS))
    for n, r in sorted(zip(names, rows)):
        if flt not in n:
            continue
        n = re.sub(r"void |\(PpGemmDesc, int, int\)", "", n)
        print(f"{n:100s} " + " ".join(f"{r.get(k, -1):7d}" for k, _ in FIELDS))
