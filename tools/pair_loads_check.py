#!/usr/bin/env python3
"""Checks the memory phase of the pair kernels in the compiled code.

usage: pair_loads_check.py <device assembly of kernels.hip>
       (hipcc --offload-arch=gfx950 <the Makefile's flags> --save-temps -c csrc/kernels.hip keeps it as
       kernels-hip-amdgcn-amd-amdhsa-gfx950.s)

dict_pair_down_kernel / dict_pair_up_kernel issue every global load before their first wait
("Pair kernels: every load at kernel entry").  Whether the compiler keeps it
that way depends on its register allocation and scheduling, so this prints, per instantiation, the
order of vector loads (L), waits on them (W) and basic-block heads (|) up to the first barrier (B),
and fails when a wait stands between two loads of one block or a kernel loads after the barrier.
A wait at the very head of a block is let through: that is the entry of the code-word form, which
the row-type form jumps over, with nothing in flight on its path (read the blocks when in doubt).
Checked with the compiler of ROCm 7.2 (AMD clang 22.0.0git): every kernel prints  ...L|L|W|B.
"""
import re
import sys


def kernels(path):
    cur, body = None, {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif cur:
            body[cur].append(line)
            if "s_endpgm" in line:
                cur = None
    return {k: v for k, v in body.items() if "dict_pair_" in k and "_kernel" in k}


def main():
    bad = 0
    found = kernels(sys.argv[1])
    if not found:
        sys.exit("no dict_pair kernel in " + sys.argv[1])
    for name, lines in found.items():
        seq, after = [], 0
        for line in lines:
            code = line.split(";")[0]
            if seq and seq[-1] == "B":
                after += bool(re.search(r"\b(global|flat|scratch)_load", code))
            elif re.search(r"\b(global|flat)_load", code):
                seq.append("L")
            elif "s_waitcnt" in code and "vmcnt" in code:
                seq.append("W")
            elif re.match(r"^\.LBB", code):
                seq.append("|")
            elif "s_barrier" in code:
                seq.append("B")
        s = re.sub(r"\|+", "|", "".join(seq))
        mid = re.search(r"LW+[|]*L", s) is not None   # a wait behind a load of its block, loads after it
        flat = sum(bool(re.search(r"\b(flat|scratch)_", l.split(";")[0])) for l in lines)
        ok = not mid and not after and not flat and (s.endswith("W|B") or s.endswith("WB"))
        bad += not ok
        tag = re.search(r"dict_pair_\w+?_kernelILi\d+ELi\d+", name).group(0)
        print(("ok   " if ok else "FAIL ") + tag, s, f"loads after the barrier: {after}, flat/scratch: {flat}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
