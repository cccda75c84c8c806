#!/usr/bin/env python3
"""One line per kernel from the remarks of `make -C cuda-optix-pathtracing_amd/csrc asm 2> asm.log`
(-Rpass-analysis=kernel-resource-usage): VGPRs, AGPRs, scratch bytes per lane, occupancy in waves per SIMD, LDS bytes per
block, spilled SGPRs and VGPRs.  Two such listings of two builds compare with diff.

Usage: python tools/kernel_resources.py asm.log > listing.txt"""
import re
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]", "SGPRs Spill", "VGPRs Spill"]


def main():
    kernels, cur = {}, None
    for line in open(sys.argv[1], errors="replace"):
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]+?): (\S+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = list(kernels)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    print(f"{'kernel':<72} {'vgpr':>5} {'agpr':>5} {'scratch':>8} {'occ':>4} {'lds':>6} {'sspill':>7} {'vspill':>7}")
    rows = []
    for name, nice in zip(names, plain):
        nice = re.sub(r"\(anonymous namespace\)::", "", nice)
        nice = re.sub(r"\(.*$", "", nice)
        rows.append((nice, [kernels[name].get(f, "?") for f in FIELDS]))
    for nice, v in sorted(rows):
        print(f"{nice:<72} {v[0]:>5} {v[1]:>5} {v[2]:>8} {v[3]:>4} {v[4]:>6} {v[5]:>7} {v[6]:>7}")


if __name__ == "__main__":
    main()
