#!/usr/bin/env python3
"""The launches of the V-cycle (double, and where the configuration says so block and float), for
comparing two builds of the library.

  run one configuration (eager: use_graph=False), vcycle(1) then vcycle(3), and print cycle_must_move()
  of parts 0 and 4 as hexadecimal floats; a configuration with the "plain" switch then runs one
  block_vcycles on 3 columns (pitch 4) and one apply_f32, and prints block_must_move(3) and
  f32_must_move() the same way; the configuration with the "slab" switch runs parts 1, 2 and 3 of the
  slab-cut cycle twice instead (amg_hip_slab_run) and prints cycle_must_move() of parts 1 to 3:
      AMG_HIP_LIBRARY=<lib.so> rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- \
          python3 tools/launch_sequence.py --config <name>
  list the configurations:
      python3 tools/launch_sequence.py --list
  compare the traces and the printed bytes of two builds (<dir>/<config>/t_kernel_trace.csv and
  <dir>/<config>.out of every configuration) and write the markdown report:
      python3 tools/launch_sequence.py --compare <dir A> <dir B> > profiles/<name>_launch_sequences.md

Only the library's existing API is used, so either build can be measured."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "algebraic-multigrid_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _configs():
    """name -> (process-wide switches, constructor); the shapes are those of the named tests"""
    import numpy as np
    import amg_ctypes as amg
    from oracle import oracle as O
    O.build()
    import test_gpu_pair_onchip as P
    import test_gpu_patch_seam as S
    import test_gpu_stencil_geometry as G

    def csc(A):
        return A.colptr, A.rowind, A.val

    cfg = {}
    for shape in ("lap256", "box300x50", "zerodiag128x50"):       # tests/test_gpu_pair_onchip.py
        for keep in (0, 1):
            cfg[f"{shape}_keep{keep}"] = ({}, lambda shape=shape, keep=keep: P._solver(amg, O, shape, bool(keep), use_graph=False))
    # tests/test_gpu_patch_seam.py: K-Patch on levels 0 .. 2, the hand-over, the seam
    cfg["lap512_patch"] = ({"patch_min_rows": 0}, lambda: S._solver(amg, O, "lap512", 1, use_graph=False))
    cfg["poisson512_tail"] = ({"tail_fusion": 1}, lambda: amg.Multigrid.poisson(
        512, 10, smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6, use_graph=False))

    def multicolor():
        A, b = O.laplacian(512), O.rhs(512)
        return amg.Multigrid(*csc(A), b, 6, smoother=amg.SM_MULTICOLOR_GS, smoother_iters=1, use_graph=False)
    cfg["multicolor512_patch"] = ({"patch_min_rows": 0}, multicolor)
    cfg["multicolor512"] = ({}, multicolor)

    def march():                                                  # tests/test_gpu_stencil_geometry.py
        op = G.box3d(*G.MARCH_SHAPES[0])
        n = op[0].size - 1
        return amg.Multigrid(*op, G.rhs_for(n), G.levels_for(n), smoother=amg.SM_JACOBI, smoother_iters=2,
                             omega=0.6, layout=amg.LAYOUT_DICT, exact_coarse_solve=True, use_graph=False)
    cfg["march64x16x3"] = ({}, march)

    def march_single():   # test_march_on_a_single_level_keeps_its_buffers: the down-leg alone, then the copy home
        op = G.box3d(64, 16, 4)
        n = op[0].size - 1
        return amg.Multigrid(*op, G.rhs_for(n), 1, smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6,
                             layout=amg.LAYOUT_DICT, keep_residual=True, exact_coarse_solve=True, use_graph=False)
    cfg["march64x16x4_single"] = ({}, march_single)

    def slab():           # tests/test_gpu_slab.py::test_slab_cycle_equals_single_gpu_cycle: rank 0 of 2, every slab level
        mg = amg.Multigrid.poisson(1024, 9, smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6, use_graph=False)
        mg.slab_setup(0, 2, -1)
        return mg
    cfg["slab1024_rank0of2"] = ({"patch_min_rows": 0, "slab": 1}, slab)
    # plain path, CSR transfers (tests/test_gpu_chebyshev.py) and tensor transfers (tests/test_gpu_line_alt.py)
    cfg["chebyshev_rs64"] = ({}, lambda: amg.Multigrid.ruge_stueben(
        *csc(O.laplacian(64)), O.rhs(64), 4, 0.25, 50, smoother=5, use_graph=False))
    cfg["line_alt_tensor64"] = ({}, lambda: amg.Multigrid.poisson_tensor(
        64, 4, smoother=7, omega=0.8, smoother_iters=1, use_graph=False))
    _plain_configs(amg, O, cfg, csc)
    return amg, cfg


def _plain_configs(amg, O, cfg, csc):
    """the configurations that also run the block and the float cycle ("plain": every switch those need):
    between them every branch of their five steps"""
    import test_gpu_block_lines as BL
    import test_gpu_pcg_project as PP
    import test_gpu_tensor_opdep as TO
    import opdep_twin
    plain = {"plain": 1}
    jac = dict(smoother=amg.SM_JACOBI, omega=0.8, use_graph=False)
    for iters in (1, 2):   # linear transfers; the copy home after an odd count
        cfg[f"plain_jacobi{iters}_poisson33"] = (plain, lambda iters=iters: amg.Multigrid.poisson(
            33, 4, smoother_iters=iters, **jac))
    for name, sm in (("chebyshev", dict(smoother=5, use_graph=False)), ("jacobi", dict(smoother_iters=2, **jac))):
        cfg[f"plain_{name}_rs64"] = (plain, lambda sm=sm: amg.Multigrid.ruge_stueben(   # CSR transfers
            *csc(O.laplacian(64)), O.rhs(64), 4, 0.25, 50, **sm))
    cfg["plain_line_alt_64x48"] = (plain, lambda: BL._alt_6448(amg, use_graph=False))
    cfg["plain_cyclic_64x48"] = (plain, lambda: BL.cyclic_solver(amg, "64x48", False))

    def opdep():           # axis levels through their CSR rows
        A, b, _ = opdep_twin.case((33, 20))
        return TO.ctor(amg, A, b, (33, 20), use_graph=False)
    cfg["plain_opdep_33x20"] = (plain, opdep)
    cfg["plain_singular_64x48"] = (plain, lambda: PP.make(amg, O, "64x48", use_graph=False)[0])  # the pinned solve
    # the four coarse kinds: one-wave band (a 4 x 4 coarsest grid), K-BandChain (2 x 2), K-Spike, K-BandWide
    cfg["plain_coarse_band"] = (plain, lambda: amg.Multigrid.poisson(129, 6, exact_coarse_solve=True, smoother_iters=2, **jac))
    cfg["plain_coarse_chain"] = (plain, lambda: amg.Multigrid.poisson(129, 7, smoother_iters=2, **jac))
    cfg["plain_coarse_spike"] = (plain, lambda: amg.Multigrid.poisson(129, 3, fast_coarse_solve=True, smoother_iters=2, **jac))
    cfg["plain_coarse_wide"] = (plain, lambda: amg.Multigrid.poisson(256, 2, smoother_iters=2, **jac))


def run(name):
    amg, cfg = _configs()
    switches, make = cfg[name]
    if "patch_min_rows" in switches:
        amg.set_patch_min_rows(switches["patch_min_rows"])
    if "tail_fusion" in switches:
        amg.set_tail_fusion(switches["tail_fusion"])
    if "plain" in switches:
        amg.set_block_lines(1)
        amg.set_f32_lines(1)
        amg.set_f32_dict(1)
    mg = make()
    try:
        if "slab" in switches:   # the ranged down-legs, the replicated rest, the ranged up-legs
            for _ in range(2):
                for part in (1, 2, 3):
                    mg.slab_run(part)
        else:
            mg.vcycle(1)
            mg.vcycle(3)
        mg.sync()
        for part in (1, 2, 3) if "slab" in switches else (0, 4):
            print(f"{name} cycle_must_move({part}) = {float(mg.cycle_must_move(part)).hex()}")
        if "plain" in switches:
            import numpy as np
            import torch
            n0 = mg.get_n_dofs(0)
            rng = np.random.default_rng(3)
            U, F = (torch.from_numpy(rng.standard_normal((n0, 3))).cuda() for _ in range(2))
            mg.block_vcycles(U, F, n=1)
            v = torch.from_numpy(rng.standard_normal(n0)).cuda()
            z = torch.empty_like(v)
            mg.apply_f32(v.data_ptr(), z.data_ptr())
            mg.sync()
            print(f"{name} coarse_solve_kind = {mg.coarse_solve_kind()}")
            print(f"{name} block_must_move(3) = {float(mg.block_must_move(3)).hex()}")
            print(f"{name} f32_must_move() = {float(mg.f32_must_move()).hex()}")
    finally:
        mg.close()


def _trace(path):
    """ordered (kernel name, grid size, workgroup size) of a rocprofv3 kernel trace"""
    files = glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"{path}: expected one kernel trace, found {files}")
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]) if "Dispatch_Id" in r else int(r["Start_Timestamp"]))
    dim = lambda r, what: "x".join(r[f"{what}_Size_{a}"] for a in "XYZ")
    return [(r["Kernel_Name"], dim(r, "Grid"), dim(r, "Workgroup")) for r in rows]


def _rle(ids):
    out = []
    for i in ids:
        if out and out[-1][0] == i:
            out[-1][1] += 1
        else:
            out.append([i, 1])
    return " ".join(f"{i}" if c == 1 else f"{i}*{c}" for i, c in out)


def compare(dir_a, dir_b):
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(dir_a, "*.out")))
    table, verdicts, body = {}, [], []
    for name in names:
        seqs, outs = [], []
        for d in (dir_a, dir_b):
            seqs.append(_trace(os.path.join(d, name)))
            with open(os.path.join(d, name + ".out")) as f:
                outs.append([line.strip() for line in f if "_must_move" in line])
        same_seq = seqs[0] == seqs[1]
        same_bytes = outs[0] == outs[1] and len(outs[0]) == (4 if name.startswith("plain_") else 3 if name.startswith("slab") else 2)
        verdicts.append((name, len(seqs[0]), len(seqs[1]), same_seq, same_bytes))
        body.append(f"### {name}\n")
        for tag, seq, out in zip("AB", seqs, outs):
            ids = [table.setdefault(k, len(table)) for k in seq]
            body.append(f"{tag}: {len(seq)} launches; " + "; ".join(out) + "\n")
            body.append("```\n" + _rle(ids) + "\n```\n")
    print("# Launch sequences of the V-cycle: parent (A) against this build (B)\n")
    print("`tools/launch_sequence.py`, one `rocprofv3 --kernel-trace` run per configuration and build: the solver is")
    print("created with `use_graph=False`, runs `vcycle(1)` and `vcycle(3)`, and prints `cycle_must_move()` of")
    print("parts 0 and 4; a `plain_*` configuration then runs one `block_vcycles` on 3 columns and one `apply_f32`")
    print("and prints `block_must_move(3)` and `f32_must_move()`; the `slab*` configuration runs `slab_run` of parts")
    print("1, 2 and 3 twice instead and prints `cycle_must_move()` of parts 1 to 3.  A list is every kernel launch of the process in")
    print("dispatch order (set-up included) as an index into the table at the end, `k*c` for c launches of k in a row.\n")
    print("| configuration | launches A | launches B | same (kernel, grid, workgroup) list | same bytes |")
    print("|---|---|---|---|---|")
    for name, na, nb, s, b in verdicts:
        print(f"| {name} | {na} | {nb} | {'yes' if s else 'NO'} | {'yes' if b else 'NO'} |")
    ok = all(s and b for *_, s, b in verdicts) and bool(verdicts)
    print(f"\n**Verdict: {'identical' if ok else 'DIFFERENT'}** over {len(verdicts)} configurations.\n")
    print("\n".join(body))
    print("## Kernels\n")
    print("| id | kernel | grid | workgroup |")
    print("|---|---|---|---|")
    for (k, g, w), i in sorted(table.items(), key=lambda kv: kv[1]):
        print(f"| {i} | `{k}` | {g} | {w} |")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if a.list:
        print("\n".join(_configs()[1]))
        return 0
    run(a.config)
    return 0


if __name__ == "__main__":
    sys.exit(main())
