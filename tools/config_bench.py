#!/usr/bin/env python3
"""Times V-cycle configurations on one GPU (the BASELINE.json configs other than the bench.py
headline) and records the convergence factor next to every rate.
usage: config_bench.py <dim> <n> <levels> <smoother> [cycles]     one configuration
       config_bench.py all                                         the README table
       config_bench.py cheb                                        the Chebyshev rows
       config_bench.py line                                        the line-smoother rows (line and Jacobi legs alternate)
       config_bench.py tensor                                      full-coarsening hierarchies next to the flat ones (legs alternate)
       config_bench.py tensor10 <n> <levels> [csr]                 ten cycles of one tensor hierarchy (kernel traces)
       config_bench.py tensor-setup [<dim> <n> <levels>]           set-up seconds of the full-coarsening hierarchy, host and device construction alternating
       config_bench.py tensor-user-setup [<nx> <ny> <nz> <levels>] set-up seconds for a variable-coefficient operator assembled on the GPU: host constructor and amg_hip_create_tensor_dev alternating
       config_bench.py alt [<nx> <ny> <levels>]                    alternating line smoother 1+1 next to true Jacobi 2+2 and the line smoother 1+1 through tensor_dev, isotropic and split-anisotropy operators (legs alternate)
       config_bench.py alt10 <nx> <ny> <levels>                    ten cycles of the alternating line smoother (kernel traces)
       config_bench.py mixed [<nx> <ny> <nz> <levels>]             amg_hip_pcg and amg_hip_pcg_mixed (single-precision V-cycle) alternating on a variable-coefficient operator, true Jacobi 2+2 and Chebyshev(2) 1+1
       config_bench.py semi [<nx> <ny> <nz> <eps_x> <eps_y> <eps_z>] PCG to 1e-8 on an axis-scaled diffusion operator: full coarsening + Jacobi, semi-coarsening + Jacobi, full coarsening + alternating lines, semi-coarsening + amg_hip_pcg_mixed (legs alternate)
       config_bench.py opdep [<nx> <ny> <nz>]                      operator-dependent interpolation (tensor_opdep) on a diffusion operator whose conductivity jumps by 10^0..10^4 between blocks of 8 nodes: ms per V-cycle with the matrix-free transfers (kind 3) against CSR transfers (kind 0), PCG to 1e-8 against full coarsening (tensor), host set-up seconds and device matrix bytes (legs alternate)
       config_bench.py opdep10 <nx> <ny> <nz> [csr]                ten cycles of one tensor_opdep hierarchy on that operator (kernel traces)
       config_bench.py opdep-setup [<nx> <ny> <nz>]                set-up seconds of tensor_opdep on that operator assembled on the GPU, explicit masks x, y, (z,) x, ...: the host constructor and amg_hip_create_tensor_opdep_dev alternating, best of three
       config_bench.py opdep-periodic [<nx> <ny> <nz>]             that operator with every axis periodic (wrap edges, singular, b of zero mean), explicit masks x, y, (z,) x, ...: tensor_opdep (wrap entries skipped), tensor_periodic (fixed weights) and tensor_opdep_periodic (the seam) alternating, all through the host constructors: PCG to 1e-8, ms per V-cycle, and the new solver with CSR transfers (amg_hip_set_axis_stencil(0))
       config_bench.py opdep-periodic-setup [<nx> <ny> <nz>]       set-up seconds of tensor_opdep_periodic_dev on the fully periodic jump operator assembled on the GPU, explicit masks x, y, (z,) x, ..., with set_periodic_device_setup off (host constructor) and on (device), legs alternate, best of three; next to them tensor_opdep_dev on the open-box operator of the same grid
       config_bench.py natural [<nx> <ny> <nz>]                    PCG to 1e-8 on a diffusion operator without a Dirichlet side (singular) and with Dirichlet on x-low only, through tensor_dev: natural_sides = 0 against the proper side mask (legs alternate)
       config_bench.py singular [<nx> <ny> <nz>]                   PCG to 1e-8 on that operator without a Dirichlet side, one solver: mean projection (amg_hip_set_mean_projection) off and on with the consistent b and on with b + 1e-6, legs alternate; the time added per iteration next to an estimate from the tree reduction's rate in the same run
       config_bench.py periodic [<nx> <ny> <nz>]                   PCG to 1e-8 on a diffusion operator with every axis periodic (singular): the periodic hierarchy (tensor_periodic_dev) against natural_sides on every side (tensor_dev), both built by the host constructor, legs alternate
       config_bench.py periodic-setup [<nx> <ny> <nz>]             set-up seconds of tensor_periodic_dev on that operator with set_periodic_device_setup off (host constructor) and on (device), legs alternate; next to them tensor_dev on the open-box operator of the same grid
       config_bench.py periodic-lines                              PCG to 1e-8 and ms per V-cycle of AMG_HIP_SM_LINE_ALT on diffusion that is strong along a periodic x axis (4096 x 1024, 256^3): open lines (cyclic_lines 0) against cyclic lines (cyclic_lines 1), legs alternate
       config_bench.py mixed-line [split2|split3|cyclic2|cyclic3]  amg_hip_pcg and amg_hip_pcg_mixed alternating on AMG_HIP_SM_LINE_ALT solvers (amg_hip_set_f32_lines): split-anisotropy through tensor_dev and the periodic-lines operator with cyclic lines, 4096 x 1024 and 256^3
       config_bench.py mixed-dict [t2|t3|c2|flat]                  amg_hip_pcg on the dictionary layout, amg_hip_pcg_mixed on a SELL solver and amg_hip_pcg_mixed on the dictionary solver (amg_hip_set_f32_dict) alternating: poisson_tensor 4096^2 and 256^3 (Jacobi 2+2), 4096^2 Chebyshev(2), poisson 4096^2 on the flat hierarchy
       config_bench.py block                                       block (multi-RHS) cycles, k = 1..16
       config_bench.py block8 rs|p4096                             one block workload at k = 8 (kernel traces)
       config_bench.py block-line [jacobi|split2|split3|cyclic2]   the line smoothers through the block entry points (amg_hip_set_block_lines) and the single-vector path alternating, k = 1..16: cycles and PCG to 1e-8
       config_bench.py block-line8 jacobi|split2|split3|cyclic2    one block-line case at k = 8, cycles only (kernel traces)
smoother: spgs | jacobi | multicolor | cheb (degree 2, 1+1) | cheb3 (degree 3, 1+1) | line (omega 0.7, 1+1).  Setup runs on the device (amg_hip_create_poisson);
smoothers that need host structures fall back to the host path inside it."""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
import amg_ctypes as amg  # noqa: E402

KW = {"spgs": dict(smoother=amg.SM_SPGS, smoother_iters=1),
      "jacobi": dict(smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6),
      "jacobi1": dict(smoother=amg.SM_JACOBI, smoother_iters=1, omega=0.6),
      "multicolor": dict(smoother=amg.SM_MULTICOLOR_GS, smoother_iters=1),
      "cheb": dict(smoother=amg.SM_CHEBYSHEV, smoother_iters=1, cheb_degree=2),
      "cheb3": dict(smoother=amg.SM_CHEBYSHEV, smoother_iters=1, cheb_degree=3),
      "line": dict(smoother=amg.SM_LINE_JACOBI, smoother_iters=1, omega=0.7)}


def run(dim, n, L, sm, cycles=10, warm=6, **extra):
    t0 = time.time()
    mg = amg.Multigrid.poisson(n, L, dim=dim, **KW[sm], **extra)
    mg.sync()
    setup = time.time() - t0
    mg.vcycle(warm)
    mg.sync()
    r0 = mg.rss()
    t1 = time.perf_counter()
    mg.vcycle(cycles)
    mg.sync()
    dt = (time.perf_counter() - t1) / cycles
    r1 = mg.rss()
    fac = (r1 / r0) ** (0.5 / cycles) if r0 > 0 and r1 > 0 else float("nan")   # per cycle, residual 2-norm
    tag = " ".join(f"{k}={v}" for k, v in extra.items())
    print(f"dim={dim} n={n} dofs={n**dim} levels={L} smoother={sm} {tag}: setup {setup:.2f}s, "
          f"{dt*1e3:.3f} ms/V-cycle = {1/dt:.1f} V-cycles/s, coarsest {mg.get_n_dofs(L-1)} dofs "
          f"(half-bw {mg.coarse_halfbw()}, {mg.coarse_solve_kind().split(' ')[0]}), "
          f"||r|| factor per cycle {fac:.4f} (rss {r0:.4e} -> {r1:.4e} over {cycles} cycles after {warm})",
          flush=True)
    mg.close()


def run_rs(n, sm, cycles=10, theta=0.25, min_coarse=500, dim=2):
    """Strength-based C/F hierarchy (amg_hip_create_rs) on the same problem; reports the cycles
    and time to reduce the residual norm by 1e-8 next to the rate."""
    cp, ri, v = amg.laplacian(n, dim)
    b = amg.rhs(n, dim)
    t0 = time.time()
    mg = amg.Multigrid.ruge_stueben(cp, ri, v, b, 25, theta, min_coarse, **KW[sm])
    mg.sync()
    setup = time.time() - t0
    L = mg.n_levels
    r0 = mg.rss()
    t1 = time.perf_counter()
    mg.vcycle(cycles)
    mg.sync()
    dt = (time.perf_counter() - t1) / cycles
    r1 = mg.rss()
    fac = (r1 / r0) ** (0.5 / cycles)
    import math
    need = math.ceil(math.log(1e-8) / math.log(fac)) if fac < 1 else float("inf")
    sizes = [mg.get_n_dofs(l) for l in range(L)]
    print(f"RS dim={dim} n={n} dofs={n**dim} levels={L} sizes={sizes[:4]}..{sizes[-1]} smoother={sm}: setup {setup:.2f}s, "
          f"{dt*1e3:.3f} ms/V-cycle = {1/dt:.1f} V-cycles/s, coarsest half-bw {mg.coarse_halfbw()}, "
          f"||r|| factor per cycle {fac:.4f}: 1e-8 in {need} cycles = {need*dt*1e3:.1f} ms", flush=True)
    if sm != "spgs":   # the V-cycle as M^-1 inside CG (reference README.md:127) from a zero guess
        mg.zero_vec(0, "u")
        mg.sync()
        t2 = time.perf_counter()
        _, it, rel = mg.pcg(1e-8, 200)
        t3 = time.perf_counter()
        print(f"   PCG on the same hierarchy: {it} iterations to relative residual {rel:.2e} in {(t3-t2)*1e3:.1f} ms "
              f"(incl. copying the solution back)", flush=True)
    mg.close()


def run_to_tol(dim, n, L, sms=("line", "jacobi"), tol=1e-8, cap=3000, reps=3, pcg_levels=None):
    """V-cycles/s, and cycles and milliseconds to ||r|| / ||r0|| <= tol from u = 0 (Grid::rhs), for
    every smoother of `sms` on the same problem, the legs alternating, `reps` repeats.  The run to
    tol checks rss every `chunk` cycles (one device synchronise per chunk) and its time is the wall
    time of the whole run, checks included.  pcg_levels: also PCG to tol on that many levels."""
    mgs = {sm: amg.Multigrid.poisson(n, L, dim=dim, **KW[sm]) for sm in sms}
    for mg in mgs.values():
        mg.vcycle(3)
        mg.sync()
    for rep_ in range(reps):
        for sm, mg in mgs.items():
            cyc = 10
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            mg.vcycle(cyc)
            mg.sync()
            dt = (time.perf_counter() - t0) / cyc
            mg.zero_vec(0, "u")
            mg.sync()
            r0 = mg.rss()
            chunk = 1 if sm == "line" else 25
            done, rel = 0, 1.0
            t1 = time.perf_counter()
            while done < cap and rel > tol:
                mg.vcycle(chunk)
                done += chunk
                rel = (mg.rss() / r0) ** 0.5
            t2 = time.perf_counter()
            arrived = "reached" if rel <= tol else "NOT reached"
            print(f"dim={dim} n={n} levels={L} {sm} rep {rep_}: {dt*1e3:.3f} ms/V-cycle = {1/dt:.1f} V-cycles/s; "
                  f"||r||/||r0|| {rel:.2e} after {done} cycles ({tol:g} {arrived}, checked every {chunk}) in "
                  f"{(t2-t1)*1e3:.1f} ms; factor per cycle {rel ** (1 / done):.4f}", flush=True)
    for mg in mgs.values():
        mg.close()
    if pcg_levels:
        for sm in sms:
            mg = amg.Multigrid.poisson(n, pcg_levels, dim=dim, **KW[sm])
            mg.pcg(1e-2, 5)                     # warm-up: graph capture
            for rep_ in range(reps):
                mg.zero_vec(0, "u")
                mg.sync()
                t0 = time.perf_counter()
                _, it, rel = mg.pcg(tol, 1000)
                t1 = time.perf_counter()
                print(f"dim={dim} n={n} levels={pcg_levels} {sm} PCG rep {rep_}: {it} iterations to {rel:.2e} in "
                      f"{(t1-t0)*1e3:.1f} ms (incl. copying the solution back)", flush=True)
            mg.close()


TENSOR_KW = {"jacobi": dict(smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.8),
             "cheb": dict(smoother=amg.SM_CHEBYSHEV, smoother_iters=1, cheb_degree=2)}


def run_tensor(n, L_tensor, L_flat, tol=1e-8, reps=3, flat_cap=200):
    """The full-coarsening hierarchy (amg_hip_create_tensor; true Jacobi omega 0.8 2+2 and Chebyshev(2)
    1+1, matrix-free transfers, and the Jacobi one again through the CSR transfer kernels) next to
    the flat hierarchy of amg_hip_create_poisson (true Jacobi 2+2, line smoother omega 0.7 1+1) on
    Grid::laplacian(n) / Grid::rhs(n), in ONE run with the legs alternating, `reps` repeats.  Per
    leg: V-cycles/s, the per-cycle factor, cycles and wall milliseconds from u = 0 to ||r|| / ||r0||
    <= tol with one rss after EVERY cycle (the flat true-Jacobi leg stops at `flat_cap` cycles, it
    needs thousands), set-up seconds, and PCG iterations and milliseconds to tol."""
    legs = {}

    def add(name, mk):
        t0 = time.time()
        mg = mk()
        mg.sync()
        legs[name] = (mg, time.time() - t0)

    add("tensor jacobi 2+2", lambda: amg.Multigrid.poisson_tensor(n, L_tensor, **TENSOR_KW["jacobi"]))
    add("tensor cheb(2) 1+1", lambda: amg.Multigrid.poisson_tensor(n, L_tensor, **TENSOR_KW["cheb"]))
    add("tensor jacobi 2+2, CSR transfers",
        lambda: amg.Multigrid.poisson_tensor(n, L_tensor, stencil_transfers=False, **TENSOR_KW["jacobi"]))
    add("flat jacobi 2+2", lambda: amg.Multigrid.poisson(n, L_flat, **KW["jacobi"]))
    add("flat line 1+1", lambda: amg.Multigrid.poisson(n, L_flat, **KW["line"]))
    for name, (mg, setup) in legs.items():
        kinds = sorted({mg.level_transfer_kind(l) for l in range(mg.n_levels - 1)})
        print(f"n={n} {name}: {mg.n_levels} levels, coarsest {mg.get_n_dofs(mg.n_levels - 1)} dofs, transfer kinds "
              f"{kinds}, setup {setup:.2f}s, must-move {mg.cycle_must_move() / 1e6:.1f} MB/cycle", flush=True)
        mg.vcycle(3)
        mg.pcg(1e-2, 3)                         # warm-up: graph captures
        mg.sync()
    for rep_ in range(reps):
        for name, (mg, _) in legs.items():
            cyc = 10
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            mg.vcycle(cyc)
            mg.sync()
            dt = (time.perf_counter() - t0) / cyc
            mg.zero_vec(0, "u")
            mg.sync()
            r0 = mg.rss()
            cap = flat_cap if name == "flat jacobi 2+2" else 100
            done, rel, prev = 0, 1.0, 1.0
            t1 = time.perf_counter()
            while done < cap and rel > tol:
                mg.vcycle(1)
                done += 1
                prev, rel = rel, (mg.rss() / r0) ** 0.5
            t2 = time.perf_counter()
            arrived = "reached" if rel <= tol else "NOT reached"
            mg.zero_vec(0, "u")
            mg.sync()
            t3 = time.perf_counter()
            _, it, prel = mg.pcg(tol, 1000)
            t4 = time.perf_counter()
            print(f"n={n} {name} rep {rep_}: {dt*1e3:.3f} ms/V-cycle = {1/dt:.1f} V-cycles/s; ||r||/||r0|| {rel:.2e} "
                  f"after {done} cycles ({tol:g} {arrived}, rss after every cycle) in {(t2-t1)*1e3:.1f} ms; factor "
                  f"per cycle {rel ** (1 / done):.4f}, last {rel / prev:.4f}; PCG {it} iterations to {prel:.2e} in "
                  f"{(t4-t3)*1e3:.1f} ms (incl. copying the solution back)", flush=True)
    for mg, _ in legs.values():
        mg.close()


def run_tensor_setup(dim, n, L, reps=3):
    """Set-up seconds of the full-coarsening Poisson hierarchy: Multigrid.poisson_tensor through the
    host constructor (generate on the host, amg_hip_create_tensor) and through the device set-up
    (amg_hip_create_poisson_tensor), alternating in one process, `reps` repeats.  Wall time around
    the constructor, closed by a device synchronise; with AMG_HIP_TIMING set the library writes
    its laps to stderr."""
    best = {}
    for rep_ in range(reps):
        for name, dev in (("host", False), ("device", True)):
            t0 = time.perf_counter()
            mg = amg.Multigrid.poisson_tensor(n, L, dim=dim, device_setup=dev, **TENSOR_KW["jacobi"])
            mg.sync()
            dt = time.perf_counter() - t0
            assert mg.setup_on_device == int(dev)
            best[name] = min(best.get(name, dt), dt)
            print(f"tensor-setup {n}^{dim} {L} levels, {name} rep {rep_}: {dt:.3f} s "
                  f"(setup_on_device {mg.setup_on_device}, coarsest {mg.get_n_dofs(L - 1)} dofs)", flush=True)
            mg.close()
    print(f"tensor-setup {n}^{dim} {L} levels: best host {best['host']:.3f} s, best device {best['device']:.3f} s, "
          f"ratio {best['host'] / best['device']:.1f}", flush=True)


def torch_diffusion(dims, seed=1, eps=None, shift=1.0, dirichlet=None):
    """-div(kappa grad u) + shift u on the grid `dims` (x fastest), kappa uniform in [1, 10] per face,
    assembled on the GPU with torch: (crow int32, col int32, val float64, b float64) device tensors in
    CSR with ascending columns.  Both triangles hold the same bits, so the arrays are the CSC arrays as
    well.  eps: a factor per axis on that axis's kappa (the scaled operator of the semi mode).
    dirichlet: mask of the sides that carry the Dirichlet face term (bit 2a = low side of axis a, bit
    2a + 1 = high side; None = every side); the other sides are natural (no face term)."""
    import torch
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    dim = len(dims)
    ext = tuple(dims) + (1,) * (3 - dim)
    n = ext[0] * ext[1] * ext[2]
    i = torch.arange(n, device=dev)
    coord = [i % ext[0], (i // ext[0]) % ext[1], i // (ext[0] * ext[1])]
    stride = [1, ext[0], ext[0] * ext[1]]
    kap = [torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 9.0 + 1.0 for _ in range(dim)]  # face i | i + stride
    w = 2 * dim + 1
    cols = torch.zeros((n, w), dtype=torch.int64, device=dev)
    vals = torch.zeros((n, w), dtype=torch.float64, device=dev)
    mask = torch.zeros((n, w), dtype=torch.bool, device=dev)
    diag = torch.full((n,), float(shift), dtype=torch.float64, device=dev)
    for a in range(dim):
        lo_ok, hi_ok = coord[a] > 0, coord[a] < ext[a] - 1
        f_lo = 5.5 if dirichlet is None or (dirichlet >> (2 * a)) & 1 else 0.0  # Dirichlet faces: 5.5
        f_hi = 5.5 if dirichlet is None or (dirichlet >> (2 * a + 1)) & 1 else 0.0
        k_lo = torch.where(lo_ok, torch.roll(kap[a], stride[a]), torch.full_like(kap[a], f_lo))
        k_hi = torch.where(hi_ok, kap[a], torch.full_like(kap[a], f_hi))
        if eps is not None:
            k_lo, k_hi = k_lo * float(eps[a]), k_hi * float(eps[a])
        diag = diag + k_lo + k_hi
        s_lo, s_hi = dim - 1 - a, dim + 1 + a  # ascending column order
        cols[:, s_lo], vals[:, s_lo], mask[:, s_lo] = i - stride[a], -k_lo, lo_ok
        cols[:, s_hi], vals[:, s_hi], mask[:, s_hi] = i + stride[a], -k_hi, hi_ok
    cols[:, dim], vals[:, dim], mask[:, dim] = i, diag, True
    crow = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    crow[1:] = torch.cumsum(mask.sum(1), 0).to(torch.int32)
    col = cols[mask].to(torch.int32).contiguous()
    val = vals[mask].contiguous()
    b = torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    return crow, col, val, b


def run_tensor_user_setup(dims, L, reps=3, tol=1e-8, cap=60):
    """Set-up seconds of the full-coarsening hierarchy of a variable-coefficient operator that was
    assembled on the GPU: the host constructor (Multigrid.tensor on host copies of the arrays; the
    copy itself is not timed) and the device set-up (Multigrid.tensor_dev on the device arrays),
    alternating in one process, `reps` repeats; wall time around the constructor, closed by a device
    synchronise.  With AMG_HIP_TIMING set the library writes its laps to stderr.  Then, once, the
    V-cycles the device-built solver needs for a residual reduction of `tol`."""
    import torch
    crow, col, val, b = torch_diffusion(dims)
    torch.cuda.synchronize()
    h = [a.cpu().numpy() for a in (crow, col, val, b)]
    tag = " x ".join(str(d) for d in dims)
    best, keep = {}, None
    for rep_ in range(reps):
        for name in ("host", "device"):
            t0 = time.perf_counter()
            if name == "host":
                mg = amg.Multigrid.tensor(h[0], h[1], h[2], h[3], dims, L, **TENSOR_KW["jacobi"])
            else:
                mg = amg.Multigrid.tensor_dev(crow, col, val, b, dims, L, **TENSOR_KW["jacobi"])
            mg.sync()
            dt = time.perf_counter() - t0
            assert mg.setup_on_device == int(name == "device")
            best[name] = min(best.get(name, dt), dt)
            print(f"tensor-user-setup {tag} {L} levels, {name} rep {rep_}: {dt:.3f} s (setup_on_device "
                  f"{mg.setup_on_device}, level-0 layout {mg.level_layout(0)}, coarsest {mg.get_n_dofs(L - 1)} dofs)",
                  flush=True)
            if name == "device" and rep_ == reps - 1:
                keep = mg
            else:
                mg.close()
    print(f"tensor-user-setup {tag} {L} levels: best host {best['host']:.3f} s, best device {best['device']:.3f} s, "
          f"ratio {best['host'] / best['device']:.1f}", flush=True)
    r0 = keep.rss()
    done, rel = 0, 1.0
    t0 = time.perf_counter()
    while rel > tol and done < cap:
        keep.vcycle(1)
        done += 1
        rel = (keep.rss() / r0) ** 0.5
    keep.sync()
    print(f"tensor-user-setup {tag}: ||r|| / ||r0|| = {rel:.2e} after {done} V-cycles (jacobi 2+2, omega 0.8), "
          f"{(time.perf_counter() - t0) * 1e3:.1f} ms including one rss per cycle", flush=True)
    keep.close()


def torch_split_anisotropy(dims, eps=1e-3):
    """5-point diffusion on the 2-D grid `dims` with harmonic-mean edge coefficients of the point
    coefficients (x, y) = (1, eps) in the left half of the domain and (eps, 1) in the right half
    (Dirichlet; a boundary edge takes the point's own coefficient), assembled on the GPU: (crow, col,
    val, b) as torch_diffusion."""
    import torch
    dev = torch.device("cuda")
    nx, ny = dims
    n = nx * ny
    i = torch.arange(n, device=dev)
    x, y = i % nx, i // nx
    left = x < nx // 2
    one, small = torch.ones(n, dtype=torch.float64, device=dev), torch.full((n,), eps, dtype=torch.float64, device=dev)
    c = [torch.where(left, one, small), torch.where(left, small, one)]
    coord, ext, stride = [x, y], [nx, ny], [1, nx]
    cols = torch.zeros((n, 5), dtype=torch.int64, device=dev)
    vals = torch.zeros((n, 5), dtype=torch.float64, device=dev)
    mask = torch.zeros((n, 5), dtype=torch.bool, device=dev)
    diag = torch.zeros(n, dtype=torch.float64, device=dev)
    for a in range(2):
        lo_ok, hi_ok = coord[a] > 0, coord[a] < ext[a] - 1
        c_lo, c_hi = torch.roll(c[a], stride[a]), torch.roll(c[a], -stride[a])
        k_lo = torch.where(lo_ok, 2.0 * c[a] * c_lo / (c[a] + c_lo), c[a])
        k_hi = torch.where(hi_ok, 2.0 * c[a] * c_hi / (c[a] + c_hi), c[a])
        diag = diag + k_lo + k_hi
        s_lo, s_hi = 1 - a, 3 + a
        cols[:, s_lo], vals[:, s_lo], mask[:, s_lo] = i - stride[a], -k_lo, lo_ok
        cols[:, s_hi], vals[:, s_hi], mask[:, s_hi] = i + stride[a], -k_hi, hi_ok
    cols[:, 2], vals[:, 2], mask[:, 2] = i, diag, True
    crow = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    crow[1:] = torch.cumsum(mask.sum(1), 0).to(torch.int32)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    b = torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    return crow, col_of(cols, mask), vals[mask].contiguous(), b


def col_of(cols, mask):
    import torch
    return cols[mask].to(torch.int32).contiguous()


ALT_KW = {"alt 1+1": dict(smoother=amg.SM_LINE_ALT, smoother_iters=1, omega=0.8),
          "jacobi 2+2": dict(smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.8),
          "line 1+1": dict(smoother=amg.SM_LINE_JACOBI, smoother_iters=1, omega=0.7)}


def run_alt(dims, L, reps=3, tol=1e-8, cap=60):
    """The alternating line smoother (omega 0.8, 1+1) next to true Jacobi (omega 0.8, 2+2) and the
    single-direction line smoother (omega 0.7, 1+1) through tensor_dev on the isotropic
    variable-coefficient operator of tensor-user-setup and on the split-anisotropy operator, the three
    legs alternating in one run, `reps` repeats.  Per leg: ms per V-cycle, and cycles and wall ms from
    u = 0 to ||r|| / ||r0|| <= tol with one rss after every cycle; a run that stops at `cap` cycles
    counts as its cap."""
    tag = " x ".join(str(d) for d in dims)
    for op, arrays in (("isotropic", torch_diffusion(dims)), ("split-anisotropy 1e-3", torch_split_anisotropy(dims))):
        legs = {}
        for name, kw in ALT_KW.items():
            t0 = time.time()
            mg = amg.Multigrid.tensor_dev(*arrays, dims, L, **kw)
            mg.sync()
            assert mg.setup_on_device == 1
            print(f"alt {tag} {L} levels {op}, {name}: setup {time.time() - t0:.2f} s, level-0 layout "
                  f"{mg.level_layout(0)}, must-move {mg.cycle_must_move() / 1e6:.1f} MB/cycle", flush=True)
            mg.vcycle(3)
            mg.sync()
            legs[name] = mg
        best = {}
        for rep_ in range(reps):
            for name, mg in legs.items():
                cyc = 10
                mg.zero_vec(0, "u")
                mg.sync()
                t0 = time.perf_counter()
                mg.vcycle(cyc)
                mg.sync()
                dt = (time.perf_counter() - t0) / cyc
                mg.zero_vec(0, "u")
                mg.sync()
                r0 = mg.rss()
                done, rel = 0, 1.0
                t1 = time.perf_counter()
                while done < cap and rel > tol:
                    mg.vcycle(1)
                    done += 1
                    rel = (mg.rss() / r0) ** 0.5
                t2 = time.perf_counter() - t1
                best[name] = min(best.get(name, t2), t2)
                print(f"alt {tag} {op}, {name} rep {rep_}: {dt * 1e3:.3f} ms/V-cycle = "
                      f"{mg.cycle_must_move() / dt / 8e12 * 100:.1f} % of 8 TB/s; ||r||/||r0|| {rel:.2e} after {done} "
                      f"cycles ({tol:g} {'reached' if rel <= tol else 'NOT reached: capped'}) in {t2 * 1e3:.1f} ms",
                      flush=True)
        print(f"alt {tag} {op}: best time to {tol:g}: " + ", ".join(f"{k} {v * 1e3:.1f} ms" for k, v in best.items()) +
              f"; alt / jacobi {best['alt 1+1'] / best['jacobi 2+2']:.3f}, alt / line "
              f"{best['alt 1+1'] / best['line 1+1']:.3f}", flush=True)
        for mg in legs.values():
            mg.close()


def run_mixed(dims, L, reps=3, rtol=1e-8, applies=10):
    """amg_hip_pcg (double V-cycle) and amg_hip_pcg_mixed (float V-cycle) to `rtol` from x = 0,
    alternating in one process, `reps` repeats, on the variable-coefficient operator of
    tensor-user-setup (tensor_dev, layout SELL), for true Jacobi 2+2 and Chebyshev(2) 1+1.  Per run:
    iterations and wall ms (the solvers synchronise themselves); then ms per preconditioner application
    over `applies` calls closed by one synchronise, and the must-move bytes of one application over
    that time as a fraction of 8 TB/s.  The double figure is the V-cycle alone (vcycle(): what
    amg_hip_pcg runs per iteration, amg_hip_cycle_must_move bytes); amg_hip_apply, which also parks and
    restores level 0's two vectors (64 bytes per row), is timed next to it.  The mixed figure is
    amg_hip_apply_f32 (what amg_hip_pcg_mixed runs per iteration, amg_hip_f32_must_move bytes)."""
    import torch
    crow, col, val, b = torch_diffusion(dims)
    torch.cuda.synchronize()
    tag = " x ".join(str(d) for d in dims)
    n = b.numel()
    z = torch.empty_like(b)
    for sm in ("jacobi", "cheb"):
        mg = amg.Multigrid.tensor_dev(crow, col, val, b, dims, L, layout=amg.LAYOUT_SELL, **TENSOR_KW[sm])
        mg.sync()
        calls = {"double": (mg.pcg, mg.apply_dev, mg.cycle_must_move()), "mixed": (mg.pcg_mixed, mg.apply_f32, None)}
        calls["mixed"] = calls["mixed"][:2] + (mg.f32_must_move(),)
        for name in calls:  # first calls: work vectors, float copies, captured graphs
            calls[name][1](b.data_ptr(), z.data_ptr())
        mg.sync()
        best = {}
        for rep_ in range(reps):
            for name, (solve, apply, mm) in calls.items():
                mg.zero_vec(0, "u")
                mg.sync()
                t0 = time.perf_counter()
                _, it, rel = solve(rtol=rtol, max_iters=100)
                dt = time.perf_counter() - t0
                t0 = time.perf_counter()
                for _ in range(applies):
                    apply(b.data_ptr(), z.data_ptr())
                mg.sync()
                da = (time.perf_counter() - t0) / applies
                extra = ""
                if name == "double":  # the cycle without amg_hip_apply's park and restore
                    mg.zero_vec(0, "u")
                    mg.sync()
                    t0 = time.perf_counter()
                    mg.vcycle(applies)
                    mg.sync()
                    extra = f" (amg_hip_apply {da * 1e3:.3f} ms)"
                    da = (time.perf_counter() - t0) / applies
                best[name] = (min(best.get(name, (dt, da))[0], dt), min(best.get(name, (dt, da))[1], da))
                print(f"mixed {tag} {L} levels {sm}, {name} rep {rep_}: {it} iterations, {dt * 1e3:.2f} ms to "
                      f"{rtol:g} (relres {rel:.2e}), {da * 1e3:.3f} ms per application{extra}, must-move {mm / 1e6:.1f} MB = "
                      f"{mm / da / 8e12 * 100:.1f} % of 8 TB/s", flush=True)
        print(f"mixed {tag} {L} levels {sm} ({n} dofs): best solve double {best['double'][0] * 1e3:.2f} ms, mixed "
              f"{best['mixed'][0] * 1e3:.2f} ms, ratio {best['double'][0] / best['mixed'][0]:.2f}; best application "
              f"double {best['double'][1] * 1e3:.3f} ms, mixed {best['mixed'][1] * 1e3:.3f} ms, ratio "
              f"{best['double'][1] / best['mixed'][1]:.2f}", flush=True)
        mg.close()


def full_levels(dims, min_coarse=32):
    """levels of the full-coarsening hierarchy that ends like the automatic semi rule: at a level of at
    most min_coarse rows or where an axis has fewer than 2 points"""
    d, nl = list(dims), 1
    while min(d) >= 2 and d[0] * d[1] * (d[2] if len(d) == 3 else 1) > min_coarse:
        d, nl = [m // 2 for m in d], nl + 1
    return nl


def run_semi(dims, eps, reps=3, rtol=1e-8, max_iters=300, theta=0.5, min_coarse=32):
    """PCG from x = 0 to `rtol` on the diffusion operator of tensor-user-setup with the conductivities
    of axis a scaled by eps[a] and mass 0.01, set up on the device, four legs alternating in one
    process, `reps` repeats: full coarsening + true Jacobi 2+2 (tensor_dev), semi-coarsening + true
    Jacobi 2+2 (tensor_semi_dev, automatic masks), full coarsening + alternating lines 1+1, and
    semi-coarsening + amg_hip_pcg_mixed (layout SELL).  Per run: iterations and wall ms of the solve (the
    solvers synchronise themselves); a leg that stops at `max_iters` counts as capped.  Once per leg:
    levels, masks, the device matrix bytes of the smoothed levels over level 0's (the operator complexity
    as the cycle pays for it) and ms per V-cycle."""
    import torch
    arrays = torch_diffusion(dims, eps=eps, shift=0.01)
    torch.cuda.synchronize()
    tag = " x ".join(str(d) for d in dims) + " eps " + "/".join(f"{e:g}" for e in eps)
    L = full_levels(dims, min_coarse)
    jac, alt = TENSOR_KW["jacobi"], ALT_KW["alt 1+1"]
    mk = {"full + jacobi": lambda: amg.Multigrid.tensor_dev(*arrays, dims, L, **jac),
          "semi + jacobi": lambda: amg.Multigrid.tensor_semi_dev(*arrays, dims, 24, theta=theta,
                                                                 min_coarse=min_coarse, **jac),
          "full + alt": lambda: amg.Multigrid.tensor_dev(*arrays, dims, L, **alt),
          "semi + mixed": lambda: amg.Multigrid.tensor_semi_dev(*arrays, dims, 24, theta=theta, min_coarse=min_coarse,
                                                                layout=amg.LAYOUT_SELL, **jac)}
    names = {1: "x", 2: "y", 3: "xy", 4: "z", 5: "xz", 6: "yz", 7: "xyz"}
    legs = {}
    for name, make in mk.items():
        t0 = time.perf_counter()
        mg = make()
        mg.sync()
        dt = time.perf_counter() - t0
        nl = mg.n_levels
        mat = [mg.level_layout(l)[1] for l in range(nl - 1)]  # the smoothed levels' matrix bytes per sweep
        masks = " ".join(names[mg.level_axes(l)] for l in range(nl - 1))
        mg.vcycle(3)
        mg.sync()
        mg.zero_vec(0, "u")
        mg.sync()
        t0 = time.perf_counter()
        mg.vcycle(10)
        mg.sync()
        cyc = (time.perf_counter() - t0) / 10
        print(f"semi {tag}, {name}: setup {dt:.2f} s (setup_on_device {mg.setup_on_device}), {nl} levels, axes [{masks}], "
              f"coarsest {mg.get_n_dofs(nl - 1)} dofs, matrix bytes of the smoothed levels / level 0 "
              f"{sum(mat) / mat[0]:.2f}, {cyc * 1e3:.3f} ms/V-cycle, "
              f"must-move {mg.cycle_must_move() / 1e6:.1f} MB", flush=True)
        solve = mg.pcg_mixed if name.endswith("mixed") else mg.pcg
        mg.zero_vec(0, "u")
        solve(rtol=rtol, max_iters=max_iters)  # first call: work vectors, float copies, captured graphs
        legs[name] = (mg, solve)
    best = {}
    for rep_ in range(reps):
        for name, (mg, solve) in legs.items():
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            _, it, rel = solve(rtol=rtol, max_iters=max_iters)
            dt = time.perf_counter() - t0
            best[name] = min(best.get(name, dt), dt)
            print(f"semi {tag}, {name} rep {rep_}: {it} iterations, {dt * 1e3:.2f} ms to {rtol:g} (relres {rel:.2e}, "
                  f"{'reached' if rel <= rtol else 'NOT reached: capped'})", flush=True)
    print(f"semi {tag}: best time to {rtol:g}: " + ", ".join(f"{k} {v * 1e3:.2f} ms" for k, v in best.items()),
          flush=True)
    for mg, _ in legs.values():
        mg.close()


def numpy_jump(dims, block=8, contrast=4, seed=7):
    """CSC arrays and a random right-hand side of the 5- / 7-point diffusion operator with Dirichlet
    sides whose conductivity is 10^k per block of `block` nodes per axis, k a random integer in
    [0, contrast]; an edge takes the k of the block of its lower endpoint, a Dirichlet side adds the
    boundary node's k to the diagonal.  Symmetric, so the CSR arrays are the CSC arrays."""
    import numpy as np
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    nb = [(m + block - 1) // block for m in dims]
    kb = 10.0 ** rng.integers(0, contrast + 1, size=nb[::-1]).astype(np.float64)
    idx = np.arange(n).reshape(dims[::-1])
    knode = kb[tuple(np.meshgrid(*[np.arange(m) // block for m in dims[::-1]], indexing="ij"))].ravel()
    diag = np.zeros(n)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [diag]
    for axis in range(len(dims)):
        ax = len(dims) - 1 - axis
        lo = np.take(idx, np.arange(dims[axis] - 1), axis=ax).ravel()
        hi = np.take(idx, np.arange(1, dims[axis]), axis=ax).ravel()
        k = knode[lo]
        np.add.at(diag, lo, k)
        np.add.at(diag, hi, k)
        for side in (0, dims[axis] - 1):
            s = np.take(idx, [side], axis=ax).ravel()
            np.add.at(diag, s, knode[s])
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [-k, -k]
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsc()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, np.random.default_rng(99).standard_normal(n)


def cyclic_masks(dims, min_coarse=32):
    """explicit single-axis masks x, y, (z,) x, ... over the axes that still have 2 points, down to a level
    of at most min_coarse rows"""
    d, masks, a = list(dims), [], 0
    while max(d) >= 2 and d[0] * d[1] * (d[2] if len(d) == 3 else 1) > min_coarse:
        if d[a] >= 2:
            masks.append(1 << a)
            d[a] //= 2
        a = (a + 1) % len(d)
    return masks


def make_opdep(arrays, dims, csr=False, cyclic=False, **kw):
    amg.set_axis_stencil(not csr)
    try:
        if cyclic:
            masks = cyclic_masks(dims)
            return amg.Multigrid.tensor_opdep(*arrays, dims, len(masks) + 1, axis_masks=masks, **TENSOR_KW["jacobi"], **kw)
        return amg.Multigrid.tensor_opdep(*arrays, dims, 40, min_coarse=32, **TENSOR_KW["jacobi"], **kw)
    finally:
        amg.set_axis_stencil(True)


def run_opdep(dims, reps=3, rtol=1e-8, max_iters=400, cycles=10):
    """The jump operator (numpy_jump, contrast 1e4), true Jacobi omega 0.8 2+2, four legs alternating
    in one process, `reps` repeats, best of them: tensor_opdep (automatic masks) with the matrix-free
    transfers (K-AxisRestrict / K-AxisProlong, kind 3), the same solver with CSR transfers
    (amg_hip_set_axis_stencil(0), kind 0, same bits), tensor_opdep with the explicit masks x, y, (z,) x, ...
    (cyclic_masks, kind 3) and full coarsening (Multigrid.tensor).  Per leg:
    host set-up seconds, levels, device matrix bytes of the smoothed levels over level 0's, ms per V-cycle
    and must-move bytes; then amg_hip_pcg from x = 0 to `rtol`: iterations and wall ms."""
    arrays = numpy_jump(dims)
    tag = " x ".join(str(d) for d in dims) + " jump 1e4"
    mk = {"opdep kind 3": lambda: make_opdep(arrays, dims),
          "opdep kind 0": lambda: make_opdep(arrays, dims, csr=True),
          "opdep cyclic masks": lambda: make_opdep(arrays, dims, cyclic=True),
          "full": lambda: amg.Multigrid.tensor(*arrays, dims, full_levels(dims), **TENSOR_KW["jacobi"])}
    legs = {}
    for name, make in mk.items():
        t0 = time.perf_counter()
        mg = make()
        mg.sync()
        dt = time.perf_counter() - t0
        nl = mg.n_levels
        mat = [mg.level_layout(l)[1] for l in range(nl - 1)]
        kinds = sorted(set(mg.level_transfer_kind(l) for l in range(nl - 1)))
        axes = "".join("xyz"[mg.level_axes(l).bit_length() - 1] if kinds != [2] else "" for l in range(nl - 1))
        mg.vcycle(3)
        mg.sync()
        print(f"opdep {tag}, {name}: host set-up {dt:.2f} s, {nl} levels, axes [{axes}], transfer kinds {kinds}, coarsest "
              f"{mg.get_n_dofs(nl - 1)} dofs, matrix bytes of the smoothed levels / level 0 {sum(mat) / mat[0]:.2f}, "
              f"must-move {mg.cycle_must_move() / 1e6:.1f} MB per V-cycle", flush=True)
        mg.zero_vec(0, "u")
        mg.pcg(rtol=rtol, max_iters=max_iters)  # first call: work vectors, captured graphs
        legs[name] = mg
    best_c, best_p, iters = {}, {}, {}
    for rep_ in range(reps):
        for name, mg in legs.items():
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            mg.vcycle(cycles)
            mg.sync()
            dt = (time.perf_counter() - t0) / cycles
            best_c[name] = min(best_c.get(name, dt), dt)
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            _, it, rel = mg.pcg(rtol=rtol, max_iters=max_iters)
            dp = time.perf_counter() - t0
            best_p[name] = min(best_p.get(name, dp), dp)
            iters[name] = it
            print(f"opdep {tag}, {name} rep {rep_}: {dt * 1e3:.3f} ms/V-cycle; PCG {it} iterations, {dp * 1e3:.2f} ms to "
                  f"{rtol:g} (relres {rel:.2e}, {'reached' if rel <= rtol else 'NOT reached: capped'})", flush=True)
    print(f"opdep {tag}: best ms/V-cycle: " + ", ".join(f"{k} {v * 1e3:.3f}" for k, v in best_c.items()) +
          "; best PCG ms: " + ", ".join(f"{k} {v * 1e3:.2f} ({iters[k]} it)" for k, v in best_p.items()), flush=True)
    for mg in legs.values():
        mg.close()


def numpy_jump_periodic(dims, block=8, contrast=4, seed=7):
    """numpy_jump's operator -- the same block conductivities from the same random stream -- with every axis
    periodic: the m edges (i, (i + 1) mod m) per grid line, the wrap edge with the k of the block of node
    m - 1, no face terms.  Singular (zero row sums); the right-hand side has zero mean."""
    import numpy as np
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    nb = [(m + block - 1) // block for m in dims]
    kb = 10.0 ** rng.integers(0, contrast + 1, size=nb[::-1]).astype(np.float64)
    idx = np.arange(n).reshape(dims[::-1])
    knode = kb[tuple(np.meshgrid(*[np.arange(m) // block for m in dims[::-1]], indexing="ij"))].ravel()
    diag = np.zeros(n)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [diag]
    for axis in range(len(dims)):
        ax = len(dims) - 1 - axis
        m = dims[axis]
        lo = np.take(idx, np.arange(m), axis=ax).ravel()
        hi = np.take(idx, (np.arange(m) + 1) % m, axis=ax).ravel()
        k = knode[lo]
        np.add.at(diag, lo, k)
        np.add.at(diag, hi, k)
        rows += [lo, hi]
        cols += [hi, lo]
        vals += [-k, -k]
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsc()
    A.sort_indices()
    b = np.random.default_rng(99).standard_normal(n)
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data, b - b.mean()


def periodic_cyclic_masks(dims, min_coarse=32):
    """cyclic_masks on a box whose axes are all periodic: an axis is halved while it is even with at least
    4 points"""
    d, masks, a, idle = list(dims), [], 0, 0
    while idle < len(d) and d[0] * d[1] * (d[2] if len(d) == 3 else 1) > min_coarse:
        if d[a] >= 4 and d[a] % 2 == 0:
            masks.append(1 << a)
            d[a] //= 2
            idle = 0
        else:
            idle += 1
        a = (a + 1) % len(d)
    return masks


def run_opdep_periodic(dims, reps=3, rtol=1e-8, max_iters=400, cycles=10):
    """The fully periodic jump operator (numpy_jump_periodic, contrast 1e4, singular), true Jacobi omega 0.8
    2+2, explicit masks x, y, (z,) x, ... (periodic_cyclic_masks), `singular`, all through the host
    constructors.  Three legs alternate in one process, `reps` repeats: tensor_opdep (the wrap entries are
    skipped; natural_sides on every side for `singular`), tensor_periodic (the fixed weights 1/2, 1, 1/2)
    and tensor_opdep_periodic (the seam); a fourth solver is the new one with CSR transfers
    (amg_hip_set_axis_stencil(0), kind 0).  Per leg: host set-up seconds apart from everything else, ms per
    V-cycle, then amg_hip_pcg from x = 0 to `rtol`: iterations and wall ms."""
    arrays = numpy_jump_periodic(dims)
    dim = len(dims)
    per, every = (1 << dim) - 1, (1 << (2 * dim)) - 1
    masks = periodic_cyclic_masks(dims)
    L = len(masks) + 1
    jac = TENSOR_KW["jacobi"]
    tag = " x ".join(str(d) for d in dims) + " periodic jump 1e4"

    def seam_csr():
        amg.set_axis_stencil(False)
        try:
            return amg.Multigrid.tensor_opdep_periodic(*arrays, dims, L, per, axis_masks=masks, singular=True, **jac)
        finally:
            amg.set_axis_stencil(True)
    mk = {"opdep, wrap skipped": lambda: amg.Multigrid.tensor_opdep(*arrays, dims, L, axis_masks=masks,
                                                                    natural_sides=every, singular=True, **jac),
          "periodic, fixed weights": lambda: amg.Multigrid.tensor_periodic(*arrays, dims, L, per, axis_masks=masks,
                                                                           singular=True, **jac),
          "opdep with the seam": lambda: amg.Multigrid.tensor_opdep_periodic(*arrays, dims, L, per, axis_masks=masks,
                                                                             singular=True, **jac),
          "opdep with the seam, kind 0": seam_csr}
    legs = {}
    for name, make in mk.items():
        t0 = time.perf_counter()
        mg = make()
        mg.sync()
        dt = time.perf_counter() - t0
        nl = mg.n_levels
        kinds = sorted(set(mg.level_transfer_kind(l) for l in range(nl - 1)))
        mg.vcycle(3)
        mg.sync()
        print(f"opdep-periodic {tag}, {name}: host set-up {dt:.2f} s (setup_on_device {mg.setup_on_device}), {nl} levels, "
              f"transfer kinds {kinds}, coarsest {mg.get_n_dofs(nl - 1)} dofs ({mg.coarse_solve_kind().split(' ')[0]}), "
              f"must-move {mg.cycle_must_move() / 1e6:.1f} MB per V-cycle", flush=True)
        mg.zero_vec(0, "u")
        mg.pcg(rtol=rtol, max_iters=max_iters)  # first call: work vectors, captured graphs
        legs[name] = mg
    cyc, pcg, iters = {k: [] for k in legs}, {k: [] for k in legs}, {}
    for rep_ in range(reps):
        for name, mg in legs.items():
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            mg.vcycle(cycles)
            mg.sync()
            dt = (time.perf_counter() - t0) / cycles
            cyc[name].append(dt)
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            _, it, rel = mg.pcg(rtol=rtol, max_iters=max_iters)
            dp = time.perf_counter() - t0
            pcg[name].append(dp)
            iters[name] = it
            print(f"opdep-periodic {tag}, {name} rep {rep_}: {dt * 1e3:.3f} ms/V-cycle; PCG {it} iterations, "
                  f"{dp * 1e3:.2f} ms to {rtol:g} (relres {rel:.2e}, {'reached' if rel <= rtol else 'NOT reached: capped'})",
                  flush=True)
    print(f"opdep-periodic {tag}: ms/V-cycle best (worst of {reps}): " +
          ", ".join(f"{k} {min(v) * 1e3:.3f} ({max(v) * 1e3:.3f})" for k, v in cyc.items()) +
          "; PCG ms best: " + ", ".join(f"{k} {min(v) * 1e3:.2f} ({iters[k]} it)" for k, v in pcg.items()), flush=True)
    for mg in legs.values():
        mg.close()


def torch_jump(dims, block=8, contrast=4, seed=7):
    """numpy_jump's operator assembled on the GPU: (crow, col, val, b) as torch_diffusion.  Only the table of
    the blocks' conductivities (a few thousand numbers, numpy_jump's generator and seed) comes from the host."""
    import numpy as np
    import torch
    dev = torch.device("cuda")
    dim = len(dims)
    n = int(np.prod(dims))
    nb = [(m + block - 1) // block for m in dims]
    kb = 10.0 ** np.random.default_rng(seed).integers(0, contrast + 1, size=nb[::-1]).astype(np.float64)
    kb = torch.from_numpy(kb.ravel()).to(dev)
    i = torch.arange(n, device=dev)
    stride = [1, dims[0], dims[0] * dims[1]][:dim]
    coord = [(i // stride[a]) % dims[a] for a in range(dim)]
    blk = torch.zeros(n, dtype=torch.int64, device=dev)
    for a in reversed(range(dim)):
        blk = blk * nb[a] + coord[a] // block
    knode = kb[blk]
    w = 2 * dim + 1
    cols = torch.zeros((n, w), dtype=torch.int64, device=dev)
    vals = torch.zeros((n, w), dtype=torch.float64, device=dev)
    mask = torch.zeros((n, w), dtype=torch.bool, device=dev)
    diag = torch.zeros(n, dtype=torch.float64, device=dev)
    for a in range(dim):
        lo_ok, hi_ok = coord[a] > 0, coord[a] < dims[a] - 1
        k_lo = torch.where(lo_ok, torch.roll(knode, stride[a]), knode)  # the edge takes the k of its lower endpoint;
        k_hi = knode                                                     # a Dirichlet side the boundary node's own
        diag = diag + k_lo + k_hi
        s_lo, s_hi = dim - 1 - a, dim + 1 + a
        cols[:, s_lo], vals[:, s_lo], mask[:, s_lo] = i - stride[a], -k_lo, lo_ok
        cols[:, s_hi], vals[:, s_hi], mask[:, s_hi] = i + stride[a], -k_hi, hi_ok
    cols[:, dim], vals[:, dim], mask[:, dim] = i, diag, True
    crow = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    crow[1:] = torch.cumsum(mask.sum(1), 0).to(torch.int32)
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    b = torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    return crow, col_of(cols, mask), vals[mask].contiguous(), b


def run_opdep_setup(dims, reps=3):
    """Set-up seconds of the hierarchy with operator-dependent interpolation on the jump operator
    (torch_jump, contrast 1e4, assembled on the GPU), explicit masks x, y, (z,) x, ... (cyclic_masks), true
    Jacobi 2+2: the host constructor (Multigrid.tensor_opdep on host copies of the arrays -- the operator is
    symmetric, its CSR arrays are its CSC arrays; the copy itself is not timed) and the device set-up
    (Multigrid.tensor_opdep_dev on the device arrays), alternating in one process, `reps` repeats, best of
    them; wall time around the constructor, closed by a device synchronise.  With AMG_HIP_TIMING set the
    library writes its laps to stderr, K-AxisWeights and K-AxisGalerkin per level among them."""
    import torch
    crow, col, val, b = torch_jump(dims)
    torch.cuda.synchronize()
    h = [a.cpu().numpy() for a in (crow, col, val, b)]
    masks = cyclic_masks(dims)
    L = len(masks) + 1
    tag = " x ".join(str(d) for d in dims) + " jump 1e4"
    best = {}
    for rep_ in range(reps):
        for name in ("host", "device"):
            t0 = time.perf_counter()
            if name == "host":
                mg = amg.Multigrid.tensor_opdep(h[0], h[1], h[2], h[3], dims, L, axis_masks=masks, **TENSOR_KW["jacobi"])
            else:
                mg = amg.Multigrid.tensor_opdep_dev(crow, col, val, b, dims, L, axis_masks=masks, **TENSOR_KW["jacobi"])
            mg.sync()
            dt = time.perf_counter() - t0
            assert mg.setup_on_device == int(name == "device")
            best[name] = min(best.get(name, dt), dt)
            kinds = sorted(set(mg.level_transfer_kind(l) for l in range(L - 1)))
            print(f"opdep-setup {tag} {L} levels, {name} rep {rep_}: {dt:.3f} s (setup_on_device {mg.setup_on_device}, "
                  f"transfer kinds {kinds}, coarsest {mg.get_n_dofs(L - 1)} dofs)", flush=True)
            mg.close()
    print(f"opdep-setup {tag} {L} levels: best host {best['host']:.3f} s, best device {best['device']:.3f} s, "
          f"ratio {best['host'] / best['device']:.1f}", flush=True)


def torch_jump_periodic(dims, block=8, contrast=4, seed=7):
    """numpy_jump_periodic's operator (every axis wraps, singular) assembled on the GPU: (crow, col, val, b) as
    torch_jump, the columns of a row ascending; b random with zero mean.  The edge (i, (i + 1) mod m) takes the
    k of the block of its lower endpoint i, the wrap edge that of node m - 1."""
    import numpy as np
    import torch
    dev = torch.device("cuda")
    dim = len(dims)
    n = int(np.prod(dims))
    nb = [(m + block - 1) // block for m in dims]
    kb = 10.0 ** np.random.default_rng(seed).integers(0, contrast + 1, size=nb[::-1]).astype(np.float64)
    kb = torch.from_numpy(kb.ravel()).to(dev)
    i = torch.arange(n, device=dev)
    stride = [1, dims[0], dims[0] * dims[1]][:dim]
    coord = [(i // stride[a]) % dims[a] for a in range(dim)]
    blk = torch.zeros(n, dtype=torch.int64, device=dev)
    for a in reversed(range(dim)):
        blk = blk * nb[a] + coord[a] // block
    knode = kb[blk]
    w = 2 * dim + 1
    cols = torch.zeros((n, w), dtype=torch.int64, device=dev)
    vals = torch.zeros((n, w), dtype=torch.float64, device=dev)
    diag = torch.zeros(n, dtype=torch.float64, device=dev)
    for a in range(dim):
        span = (dims[a] - 1) * stride[a]
        lo = torch.where(coord[a] > 0, i - stride[a], i + span)
        hi = torch.where(coord[a] < dims[a] - 1, i + stride[a], i - span)
        k_lo, k_hi = knode[lo], knode
        diag = diag + k_lo + k_hi
        cols[:, 2 * a], vals[:, 2 * a] = lo, -k_lo
        cols[:, 2 * a + 1], vals[:, 2 * a + 1] = hi, -k_hi
    cols[:, 2 * dim], vals[:, 2 * dim] = i, diag
    cols, order = torch.sort(cols, dim=1)
    vals = torch.gather(vals, 1, order)
    crow = (torch.arange(n + 1, device=dev) * w).to(torch.int32)
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    b = torch.randn(n, generator=g, device=dev, dtype=torch.float64)
    return crow, cols.reshape(-1).to(torch.int32).contiguous(), vals.reshape(-1).contiguous(), b - b.mean()


def run_opdep_periodic_setup(dims, reps=3):
    """Set-up seconds of Multigrid.tensor_opdep_periodic_dev on the fully periodic jump operator
    (torch_jump_periodic, contrast 1e4, singular, assembled on the GPU), explicit masks x, y, (z,) x, ...
    (periodic_cyclic_masks), true Jacobi 2+2, with amg_hip_set_periodic_device_setup off -- the arrays are
    downloaded and take the host constructor -- and on -- K-AxisWeights / K-AxisGalerkin with the seam.  The
    legs alternate in one process, `reps` repeats, best of them; wall time around the constructor, closed by
    a device synchronise.  Next to them, in the same loop, Multigrid.tensor_opdep_dev on the open-box jump
    operator (torch_jump) of the same grid with the same masks: the set-up without a seam.  With
    AMG_HIP_TIMING set the library writes its laps to stderr, the two kernels per level among them."""
    import torch
    dim = len(dims)
    per = (1 << dim) - 1
    arrays = torch_jump_periodic(dims)
    box = torch_jump(dims)
    torch.cuda.synchronize()
    masks = periodic_cyclic_masks(dims)
    L = len(masks) + 1
    jac = TENSOR_KW["jacobi"]
    tag = " x ".join(str(d) for d in dims) + " periodic jump 1e4"
    legs = (("switch off", 0, 0, lambda: amg.Multigrid.tensor_opdep_periodic_dev(*arrays, dims, L, per, axis_masks=masks,
                                                                                 singular=True, **jac)),
            ("switch on", 1, 1, lambda: amg.Multigrid.tensor_opdep_periodic_dev(*arrays, dims, L, per, axis_masks=masks,
                                                                                singular=True, **jac)),
            ("open box tensor_opdep_dev", 0, 1, lambda: amg.Multigrid.tensor_opdep_dev(*box, dims, L, axis_masks=masks,
                                                                                       **jac)))
    best = {}
    try:
        for rep_ in range(reps):
            for name, on, on_device, make in legs:
                amg.set_periodic_device_setup(on)
                t0 = time.perf_counter()
                mg = make()
                mg.sync()
                dt = time.perf_counter() - t0
                assert mg.setup_on_device == on_device, (name, mg.setup_on_device)
                best[name] = min(best.get(name, dt), dt)
                kinds = sorted(set(mg.level_transfer_kind(l) for l in range(L - 1)))
                print(f"opdep-periodic-setup {tag} {L} levels, {name} rep {rep_}: {dt:.3f} s (setup_on_device "
                      f"{mg.setup_on_device}, transfer kinds {kinds}, coarsest {mg.get_n_dofs(L - 1)} dofs)", flush=True)
                mg.close()
    finally:
        amg.set_periodic_device_setup(0)
    off, on, box_t = best["switch off"], best["switch on"], best["open box tensor_opdep_dev"]
    print(f"opdep-periodic-setup {tag} {L} levels: best switch off {off:.3f} s, best switch on {on:.3f} s, ratio "
          f"{off / on:.1f}; open box tensor_opdep_dev {box_t:.3f} s, switch on / open box {on / box_t:.2f}", flush=True)


def run_natural(dims, reps=3, rtol=1e-8, max_iters=300):
    """PCG from x = 0 to `rtol` on the diffusion operator of tensor-user-setup without mass term, full
    coarsening, true Jacobi 2+2, set up on the device (tensor_dev): once without a Dirichlet side (A is
    singular, b has zero mean) and once with Dirichlet on x-low only.  Two legs per operator alternate in
    one process, `reps` repeats: natural_sides = 0 (the hierarchy of the Dirichlet box) and the proper
    side mask (with singular = 1 on the first operator).  Per run: iterations and wall ms of amg_hip_pcg
    itself (it synchronises before it returns); the copy of x to the host, whose time scatters by more
    than a short solve takes, stays outside the clock."""
    import ctypes
    import torch

    def solve(mg):
        it, rel = ctypes.c_int64(0), ctypes.c_double(0)
        st = amg.lib().amg_hip_pcg(mg._h, rtol, max_iters, ctypes.byref(it), ctypes.byref(rel))
        assert st == 0, amg.lib().amg_hip_last_error().decode()
        return it.value, rel.value

    dim = len(dims)
    every = (1 << (2 * dim)) - 1
    L = full_levels(dims)
    tag = " x ".join(str(d) for d in dims)
    for what, dirichlet in (("no Dirichlet side", 0), ("Dirichlet on x-low", 1)):
        crow, col, val, b = torch_diffusion(dims, shift=0.0, dirichlet=dirichlet)
        if not dirichlet:
            b = b - b.mean()
        torch.cuda.synchronize()
        sides = every & ~dirichlet
        legs = {}
        for name, kw in (("natural_sides 0", dict()),
                         (f"natural_sides {sides}", dict(natural_sides=sides, singular=not dirichlet))):
            t0 = time.perf_counter()
            mg = amg.Multigrid.tensor_dev(crow, col, val, b, dims, L, **TENSOR_KW["jacobi"], **kw)
            mg.sync()
            dt = time.perf_counter() - t0
            mg.vcycle(3)
            mg.sync()
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            mg.vcycle(10)
            mg.sync()
            cyc = (time.perf_counter() - t0) / 10
            print(f"natural {tag}, {what}, {name}: setup {dt:.2f} s (setup_on_device {mg.setup_on_device}), "
                  f"{mg.n_levels} levels, coarsest {mg.get_n_dofs(mg.n_levels - 1)} dofs "
                  f"({mg.coarse_solve_kind().split(' ')[0]}), {cyc * 1e3:.3f} ms/V-cycle", flush=True)
            mg.zero_vec(0, "u")
            solve(mg)  # first call: work vectors, captured graph
            legs[name] = mg
        best = {}
        for rep_ in range(reps):
            for name, mg in legs.items():
                mg.zero_vec(0, "u")
                mg.sync()
                t0 = time.perf_counter()
                it, rel = solve(mg)
                dt = time.perf_counter() - t0
                best[name] = min(best.get(name, (it, dt)), (it, dt), key=lambda v: v[1])
                print(f"natural {tag}, {what}, {name} rep {rep_}: {it} iterations, {dt * 1e3:.2f} ms to {rtol:g} "
                      f"(relres {rel:.2e}, {'reached' if rel <= rtol else 'NOT reached: capped'})", flush=True)
        print(f"natural {tag}, {what}: best to {rtol:g}: " +
              ", ".join(f"{k} {v[0]} iterations {v[1] * 1e3:.2f} ms" for k, v in best.items()), flush=True)
        for mg in legs.values():
            mg.close()


def run_singular(dims, reps=3, rtol=1e-8, max_iters=60):
    """Mean projection (amg_hip_set_mean_projection) on run_natural's operator without a Dirichlet side: full
    coarsening, true Jacobi 2+2, all sides natural, singular, set up on the device (tensor_dev).  ONE solver,
    amg_hip_pcg from x = 0 to `rtol`, three legs alternating in one process, `reps` repeats: the switch off
    and on with the consistent b (zero mean), and on with b + 1e-6.  Per leg the best run: iterations, wall ms
    of amg_hip_pcg itself (it synchronises before it returns), ms per iteration, and for the legs with the
    switch on the ms per iteration added to the off leg of the same run.
    Held against: two more level-0 vector passes per iteration (the tree sum of z reads 8 n0 bytes, the
    fused centring stores 8 n0 bytes that launch_dot does not) at the rate of the library's tree reduction
    in this run, and two more launches at 4.6 us.  The rate: amg_hip_dev_sumsq
    (launch_sum) over 2 n0 doubles, which moves the 16 n0 bytes of launch_dot(n0) through the same grid,
    grid-stride order and tree as one stream instead of two; best of 20 after a warm-up, each timed
    through a device synchronise."""
    import ctypes
    import torch

    def solve(mg):
        it, rel = ctypes.c_int64(0), ctypes.c_double(0)
        st = amg.lib().amg_hip_pcg(mg._h, rtol, max_iters, ctypes.byref(it), ctypes.byref(rel))
        assert st == 0, amg.lib().amg_hip_last_error().decode()
        return it.value, rel.value

    dim = len(dims)
    every = (1 << (2 * dim)) - 1
    L = full_levels(dims)
    tag = " x ".join(str(d) for d in dims)
    crow, col, val, b = torch_diffusion(dims, shift=0.0, dirichlet=0)
    b = b - b.mean()
    b_off = b + 1e-6
    n0 = b.numel()
    torch.cuda.synchronize()
    mg = amg.Multigrid.tensor_dev(crow, col, val, b, dims, L, **TENSOR_KW["jacobi"], natural_sides=every, singular=True)
    mg.sync()
    print(f"singular {tag}: {n0} rows, {mg.n_levels} levels, coarsest {mg.get_n_dofs(mg.n_levels - 1)} dofs "
          f"({mg.coarse_solve_kind().split(' ')[0]}), setup_on_device {mg.setup_on_device}", flush=True)
    # the rate of the tree reduction over 16 n0 bytes
    two = torch.rand(2 * n0, device="cuda", dtype=torch.float64)
    out = torch.zeros(1, device="cuda", dtype=torch.float64)
    scratch = torch.zeros(1100, device="cuda", dtype=torch.float64)
    red = []
    for k in range(23):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = amg.lib().amg_hip_dev_sumsq(2 * n0, two.data_ptr(), out.data_ptr(), scratch.data_ptr(), None)
        torch.cuda.synchronize()
        assert st == 0
        if k >= 3:
            red.append(time.perf_counter() - t0)
    t_red = min(red)
    rate = 16.0 * n0 / t_red
    estimate = 16.0 * n0 / rate + 2 * 4.6e-6
    print(f"singular {tag}: tree reduction over 16 n0 = {16 * n0 / 1e6:.1f} MB: {t_red * 1e3:.4f} ms with its two "
          f"launches and the synchronise ({rate / 1e9:.0f} GB/s); estimate of the addition per iteration "
          f"{estimate * 1e3:.4f} ms", flush=True)
    legs = (("off, b", 0, b), ("on, b", 1, b), ("on, b + 1e-6", 1, b_off))
    for name, on, rhs in legs:  # first calls: work vectors, captured graph, code objects
        mg.set_mean_projection(on)
        mg.copy_vec_dev(0, "f", rhs.data_ptr(), True)
        mg.zero_vec(0, "u")
        solve(mg)
    best = {}
    for rep_ in range(reps):
        for name, on, rhs in legs:
            mg.set_mean_projection(on)
            mg.copy_vec_dev(0, "f", rhs.data_ptr(), True)
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            it, rel = solve(mg)
            dt = time.perf_counter() - t0
            best[name] = min(best.get(name, (it, dt, rel)), (it, dt, rel), key=lambda v: v[1])
            print(f"singular {tag}, {name} rep {rep_}: {it} iterations, {dt * 1e3:.2f} ms to {rtol:g} "
                  f"(relres {rel:.2e}, {'reached' if rel <= rtol else 'NOT reached: capped'})", flush=True)
    per_off = best["off, b"][1] / max(best["off, b"][0], 1)
    for name, _, _ in legs:
        it, dt, rel = best[name]
        per = dt / max(it, 1)
        line = f"singular {tag}, {name}: best {it} iterations, {dt * 1e3:.2f} ms, {per * 1e3:.4f} ms/iteration"
        if name != "off, b":
            add = per - per_off
            line += (f", added {add * 1e3:+.4f} ms/iteration ({add / estimate:.2f} x the estimate "
                     f"{estimate * 1e3:.4f} ms)")
        print(line, flush=True)
    # what the switch is for: the same b + 1e-6 with the switch off
    mg.set_mean_projection(0)
    mg.copy_vec_dev(0, "f", b_off.data_ptr(), True)
    mg.zero_vec(0, "u")
    it, rel = solve(mg)
    x = mg.get_soln(0)
    print(f"singular {tag}, off, b + 1e-6: {it} iterations, relres {rel:.2e} "
          f"({'reached' if rel <= rtol else 'NOT reached: capped'}), max|x| {abs(x).max():.2e}", flush=True)
    mg.close()


def torch_periodic_diffusion(dims, periodic, seed=1):
    """torch_diffusion without mass term and without Dirichlet faces whose axes of the mask `periodic`
    (bit a = axis a) wrap around: point m - 1 is coupled to point 0 through the face conductivity stored
    at m - 1.  The wrap entries do not sit in stencil order, so the columns of a row are sorted.  Both
    triangles hold the same bits.  An axis of fewer than 3 points cannot be periodic here (its two
    couplings would share a column)."""
    import torch
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    dim = len(dims)
    ext = tuple(dims) + (1,) * (3 - dim)
    assert all(ext[a] >= 3 for a in range(dim) if (periodic >> a) & 1)
    n = ext[0] * ext[1] * ext[2]
    i = torch.arange(n, device=dev)
    coord = [i % ext[0], (i // ext[0]) % ext[1], i // (ext[0] * ext[1])]
    stride = [1, ext[0], ext[0] * ext[1]]
    kap = [torch.rand(n, generator=g, device=dev, dtype=torch.float64) * 9.0 + 1.0 for _ in range(dim)]  # face i | next
    w = 2 * dim + 1
    cols = torch.full((n, w), n, dtype=torch.int64, device=dev)  # n: no entry, sorts last
    vals = torch.zeros((n, w), dtype=torch.float64, device=dev)
    diag = torch.zeros((n,), dtype=torch.float64, device=dev)
    for a in range(dim):
        per = bool((periodic >> a) & 1)
        first, last = coord[a] == 0, coord[a] == ext[a] - 1
        lo = torch.where(first, i + (ext[a] - 1) * stride[a], i - stride[a])
        hi = torch.where(last, i - (ext[a] - 1) * stride[a], i + stride[a])
        lo_ok = ~first if not per else torch.ones_like(first)
        hi_ok = ~last if not per else torch.ones_like(last)
        k_lo = torch.where(lo_ok, kap[a][lo], torch.zeros_like(kap[a]))
        k_hi = torch.where(hi_ok, kap[a], torch.zeros_like(kap[a]))
        diag = diag + k_lo + k_hi
        cols[:, 2 * a] = torch.where(lo_ok, lo, cols[:, 2 * a])
        cols[:, 2 * a + 1] = torch.where(hi_ok, hi, cols[:, 2 * a + 1])
        vals[:, 2 * a], vals[:, 2 * a + 1] = -k_lo, -k_hi
    cols[:, w - 1], vals[:, w - 1] = i, diag
    cols, order = torch.sort(cols, dim=1)
    vals = torch.gather(vals, 1, order)
    mask = cols < n
    crow = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    crow[1:] = torch.cumsum(mask.sum(1), 0).to(torch.int32)
    col = cols[mask].to(torch.int32).contiguous()
    val = vals[mask].contiguous()
    b = torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    return crow, col, val, b - b.mean()


def periodic_levels(dims, min_coarse=32):
    """levels of the full-coarsening hierarchy of a box whose axes are all periodic: coarsen while the
    level has more than min_coarse rows and every axis is even with at least 4 points"""
    d, nl = list(dims), 1
    while all(m >= 4 and m % 2 == 0 for m in d) and d[0] * d[1] * (d[2] if len(d) == 3 else 1) > min_coarse:
        d, nl = [m // 2 for m in d], nl + 1
    return nl


def run_periodic(dims, reps=3, rtol=1e-8, max_iters=300):
    """PCG from x = 0 to `rtol` on the diffusion operator of tensor-user-setup without mass term whose
    axes are all periodic (A is singular, b has zero mean), full coarsening, true Jacobi 2+2.  Two legs
    alternate in one process, `reps` repeats: the periodic hierarchy (tensor_periodic_dev) and the best
    hierarchy without it, natural_sides on every side with singular = 1 (tensor_dev).  Both are built by
    the host constructor (setup_on_device 0): tensor_dev leaves its device path on an operator with wrap
    entries.  Per run: iterations and wall ms of amg_hip_pcg itself; once per
    leg: set-up seconds and ms per V-cycle."""
    import ctypes
    import torch

    def solve(mg):
        it, rel = ctypes.c_int64(0), ctypes.c_double(0)
        st = amg.lib().amg_hip_pcg(mg._h, rtol, max_iters, ctypes.byref(it), ctypes.byref(rel))
        assert st == 0, amg.lib().amg_hip_last_error().decode()
        return it.value, rel.value

    dim = len(dims)
    per, every = (1 << dim) - 1, (1 << (2 * dim)) - 1
    L = periodic_levels(dims)
    tag = " x ".join(str(d) for d in dims)
    arrays = torch_periodic_diffusion(dims, per)
    torch.cuda.synchronize()
    jac = TENSOR_KW["jacobi"]
    mk = {f"periodic_axes {per}": lambda: amg.Multigrid.tensor_periodic_dev(*arrays, dims, L, per, singular=True, **jac),
          f"natural_sides {every}": lambda: amg.Multigrid.tensor_dev(*arrays, dims, L, natural_sides=every,
                                                                     singular=True, **jac)}
    legs = {}
    for name, make in mk.items():
        t0 = time.perf_counter()
        mg = make()
        mg.sync()
        dt = time.perf_counter() - t0
        mg.vcycle(3)
        mg.sync()
        mg.zero_vec(0, "u")
        mg.sync()
        t0 = time.perf_counter()
        mg.vcycle(10)
        mg.sync()
        cyc = (time.perf_counter() - t0) / 10
        print(f"periodic {tag}, {name}: setup {dt:.2f} s (setup_on_device {mg.setup_on_device}), "
              f"{mg.n_levels} levels, coarsest {mg.get_n_dofs(mg.n_levels - 1)} dofs "
              f"({mg.coarse_solve_kind().split(' ')[0]}), {cyc * 1e3:.3f} ms/V-cycle", flush=True)
        mg.zero_vec(0, "u")
        solve(mg)  # first call: work vectors, captured graph
        legs[name] = mg
    best = {}
    for rep_ in range(reps):
        for name, mg in legs.items():
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            it, rel = solve(mg)
            dt = time.perf_counter() - t0
            best[name] = min(best.get(name, (it, dt)), (it, dt), key=lambda v: v[1])
            print(f"periodic {tag}, {name} rep {rep_}: {it} iterations, {dt * 1e3:.2f} ms to {rtol:g} "
                  f"(relres {rel:.2e}, {'reached' if rel <= rtol else 'NOT reached: capped'})", flush=True)
    print(f"periodic {tag}: best to {rtol:g}: " +
          ", ".join(f"{k} {v[0]} iterations {v[1] * 1e3:.2f} ms" for k, v in best.items()), flush=True)
    for mg in legs.values():
        mg.close()


def run_periodic_setup(dims, reps=3):
    """Set-up seconds of Multigrid.tensor_periodic_dev on run_periodic's operator (every axis periodic,
    singular, true Jacobi 2+2 omega 0.8, full coarsening) with amg_hip_set_periodic_device_setup off --
    the arrays are downloaded and take the host constructor -- and on -- the level loop on the device
    with K-TensorGalerkin's periodic form.  The two legs alternate in one process, `reps` repeats; wall
    time around the constructor, closed by a device synchronise.  Next to them, in the same loop,
    Multigrid.tensor_dev on the open-box operator of tensor-user-setup on the same grid with the same
    number of levels: the product without a seam."""
    import torch
    dim = len(dims)
    per = (1 << dim) - 1
    L = periodic_levels(dims)
    tag = " x ".join(str(d) for d in dims)
    arrays = torch_periodic_diffusion(dims, per)
    box = torch_diffusion(dims)
    torch.cuda.synchronize()
    jac = TENSOR_KW["jacobi"]
    legs = (("switch off", 0, lambda: amg.Multigrid.tensor_periodic_dev(*arrays, dims, L, per, singular=True, **jac)),
            ("switch on", 1, lambda: amg.Multigrid.tensor_periodic_dev(*arrays, dims, L, per, singular=True, **jac)),
            ("open box tensor_dev", 0, lambda: amg.Multigrid.tensor_dev(*box, dims, L, **jac)))
    best = {}
    try:
        for rep_ in range(reps):
            for name, on, make in legs:
                amg.set_periodic_device_setup(on)
                t0 = time.perf_counter()
                mg = make()
                mg.sync()
                dt = time.perf_counter() - t0
                best[name] = min(best.get(name, dt), dt)
                print(f"periodic-setup {tag} {L} levels, {name} rep {rep_}: {dt:.3f} s (setup_on_device "
                      f"{mg.setup_on_device}, level-0 layout {mg.level_layout(0)}, coarsest {mg.get_n_dofs(L - 1)} dofs)",
                      flush=True)
                mg.close()
    finally:
        amg.set_periodic_device_setup(0)
    off, on, box_t = best["switch off"], best["switch on"], best["open box tensor_dev"]
    print(f"periodic-setup {tag} {L} levels: best switch off {off:.3f} s, best switch on {on:.3f} s, ratio "
          f"{off / on:.1f}; open box tensor_dev {box_t:.3f} s, switch on / open box {on / box_t:.2f}", flush=True)


def torch_scaled_periodic(dims, eps, periodic):
    """Constant-coefficient diffusion on the device as CSR: eps[a] times (-1, 2, -1) along axis a, the
    axes of the mask `periodic` wrap around, every other side is Dirichlet; b random."""
    import torch
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    dim = len(dims)
    ext = tuple(dims) + (1,) * (3 - dim)
    assert all(ext[a] >= 3 for a in range(dim) if (periodic >> a) & 1)
    n = ext[0] * ext[1] * ext[2]
    i = torch.arange(n, device=dev)
    coord = [i % ext[0], (i // ext[0]) % ext[1], i // (ext[0] * ext[1])]
    stride = [1, ext[0], ext[0] * ext[1]]
    w = 2 * dim + 1
    cols = torch.full((n, w), n, dtype=torch.int64, device=dev)  # n: no entry, sorts last
    vals = torch.zeros((n, w), dtype=torch.float64, device=dev)
    for a in range(dim):
        per = bool((periodic >> a) & 1)
        first, last = coord[a] == 0, coord[a] == ext[a] - 1
        lo = torch.where(first, i + (ext[a] - 1) * stride[a], i - stride[a])
        hi = torch.where(last, i - (ext[a] - 1) * stride[a], i + stride[a])
        lo_ok = ~first if not per else torch.ones_like(first)
        hi_ok = ~last if not per else torch.ones_like(last)
        cols[:, 2 * a] = torch.where(lo_ok, lo, cols[:, 2 * a])
        cols[:, 2 * a + 1] = torch.where(hi_ok, hi, cols[:, 2 * a + 1])
        vals[:, 2 * a] = torch.where(lo_ok, -float(eps[a]), 0.0)
        vals[:, 2 * a + 1] = torch.where(hi_ok, -float(eps[a]), 0.0)
    cols[:, w - 1], vals[:, w - 1] = i, 2.0 * float(sum(eps[:dim]))
    cols, order = torch.sort(cols, dim=1)
    vals = torch.gather(vals, 1, order)
    mask = cols < n
    crow = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    crow[1:] = torch.cumsum(mask.sum(1), 0).to(torch.int32)
    col = cols[mask].to(torch.int32).contiguous()
    val = vals[mask].contiguous()
    b = torch.rand(n, generator=g, device=dev, dtype=torch.float64) - 0.5
    return crow, col, val, b


def run_periodic_lines(dims, eps, L, reps=3, rtol=1e-8, max_iters=300):
    """AMG_HIP_SM_LINE_ALT 1+1 omega 0.8 on axis-scaled diffusion, x periodic and strongly coupled, every
    other side Dirichlet, full coarsening with L levels: open lines (cyclic_lines 0) next to cyclic lines
    (cyclic_lines 1: K-LineSeam between the residual and the solve of every x sub-sweep).  The two legs
    alternate in one process, `reps` repeats.  Per run: iterations and wall ms of amg_hip_pcg itself;
    once per leg: set-up seconds, ms per V-cycle (their difference is the cost of K-LineSeam) and the
    bytes one cycle has to move."""
    import ctypes
    import torch

    def solve(mg):
        it, rel = ctypes.c_int64(0), ctypes.c_double(0)
        st = amg.lib().amg_hip_pcg(mg._h, rtol, max_iters, ctypes.byref(it), ctypes.byref(rel))
        assert st == 0, amg.lib().amg_hip_last_error().decode()
        return it.value, rel.value

    tag = " x ".join(str(d) for d in dims)
    arrays = torch_scaled_periodic(dims, eps, 1)
    torch.cuda.synchronize()
    legs = {}
    for cyc in (0, 1):
        name = f"cyclic_lines {cyc}"
        t0 = time.perf_counter()
        mg = amg.Multigrid.tensor_periodic_dev(*arrays, dims, L, 1, cyclic_lines=cyc, **ALT_KW["alt 1+1"])
        mg.sync()
        dt = time.perf_counter() - t0
        mg.vcycle(3)
        mg.sync()
        best_cyc = float("inf")
        for _ in range(reps):
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            mg.vcycle(10)
            mg.sync()
            best_cyc = min(best_cyc, (time.perf_counter() - t0) / 10)
        print(f"periodic-lines {tag} eps {eps}, {name}: setup {dt:.2f} s (setup_on_device {mg.setup_on_device}), "
              f"{mg.n_levels} levels, cyclic axes per level {[mg.line_cyclic(l) for l in range(mg.n_levels)]}, "
              f"{best_cyc * 1e3:.3f} ms/V-cycle (best of {reps} x 10), must move {mg.cycle_must_move() / 1e6:.1f} MB",
              flush=True)
        mg.zero_vec(0, "u")
        solve(mg)  # first call: work vectors, captured graph
        legs[name] = (mg, best_cyc)
    best = {}
    for rep_ in range(reps):
        for name, (mg, _) in legs.items():
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            it, rel = solve(mg)
            dt = time.perf_counter() - t0
            best[name] = min(best.get(name, (it, dt)), (it, dt), key=lambda v: v[1])
            print(f"periodic-lines {tag}, {name} rep {rep_}: {it} iterations, {dt * 1e3:.2f} ms to {rtol:g} "
                  f"(relres {rel:.2e}, {'reached' if rel <= rtol else 'NOT reached: capped'})", flush=True)
    c0, c1 = legs["cyclic_lines 0"][1], legs["cyclic_lines 1"][1]
    print(f"periodic-lines {tag}: best to {rtol:g}: " +
          ", ".join(f"{k} {v[0]} iterations {v[1] * 1e3:.2f} ms" for k, v in best.items()) +
          f"; V-cycle {c0 * 1e3:.3f} -> {c1 * 1e3:.3f} ms (K-LineSeam {(c1 - c0) * 1e3:+.3f} ms, {(c1 / c0 - 1) * 100:+.1f} %)",
          flush=True)
    for mg, _ in legs.values():
        mg.close()


def torch_split_anisotropy_nd(dims, eps=1e-3):
    """torch_split_anisotropy in 2-D or 3-D: point coefficients (x, y) = (1, eps) in the left half of the
    box and (eps, 1) in the right half, z = eps everywhere (one strong direction at every point);
    harmonic means on the edges, Dirichlet; (crow, col, val, b) on the GPU."""
    import torch
    dev = torch.device("cuda")
    dim = len(dims)
    ext = tuple(dims) + (1,) * (3 - dim)
    n = ext[0] * ext[1] * ext[2]
    i = torch.arange(n, device=dev)
    coord = [i % ext[0], (i // ext[0]) % ext[1], i // (ext[0] * ext[1])]
    stride = [1, ext[0], ext[0] * ext[1]]
    left = coord[0] < ext[0] // 2
    one, small = torch.ones(n, dtype=torch.float64, device=dev), torch.full((n,), eps, dtype=torch.float64, device=dev)
    c = [torch.where(left, one, small), torch.where(left, small, one), small]
    w = 2 * dim + 1
    cols = torch.full((n, w), n, dtype=torch.int64, device=dev)  # n: no entry, sorts last
    vals = torch.zeros((n, w), dtype=torch.float64, device=dev)
    diag = torch.zeros(n, dtype=torch.float64, device=dev)
    for a in range(dim):
        lo_ok, hi_ok = coord[a] > 0, coord[a] < ext[a] - 1
        c_lo, c_hi = torch.roll(c[a], stride[a]), torch.roll(c[a], -stride[a])
        k_lo = torch.where(lo_ok, 2.0 * c[a] * c_lo / (c[a] + c_lo), c[a])
        k_hi = torch.where(hi_ok, 2.0 * c[a] * c_hi / (c[a] + c_hi), c[a])
        diag = diag + k_lo + k_hi
        cols[:, 2 * a] = torch.where(lo_ok, i - stride[a], cols[:, 2 * a])
        cols[:, 2 * a + 1] = torch.where(hi_ok, i + stride[a], cols[:, 2 * a + 1])
        vals[:, 2 * a], vals[:, 2 * a + 1] = -k_lo, -k_hi
    cols[:, w - 1], vals[:, w - 1] = i, diag
    cols, order = torch.sort(cols, dim=1)
    vals = torch.gather(vals, 1, order)
    mask = cols < n
    crow = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    crow[1:] = torch.cumsum(mask.sum(1), 0).to(torch.int32)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    b = torch.rand(n, generator=g, device=dev, dtype=torch.float64)
    return crow, cols[mask].to(torch.int32).contiguous(), vals[mask].contiguous(), b


def run_mixed_line(label, make, reps=3, rtol=1e-8, applies=10):
    """amg_hip_pcg (double cycle) and amg_hip_pcg_mixed (float cycle, amg_hip_set_f32_lines) to `rtol` from
    x = 0 on one AMG_HIP_SM_LINE_ALT solver (omega 0.8, 1+1, layout SELL) made by make(), alternating in one
    process, best of `reps`.  Per run: iterations and wall ms; then ms per preconditioner application over
    `applies` calls closed by one synchronise (double: vcycle(), the cycle amg_hip_pcg runs; mixed:
    amg_hip_apply_f32) and the must-move bytes of one application over that time as a share of 8 TB/s."""
    import torch
    t0 = time.perf_counter()
    mg, b = make()
    mg.sync()
    print(f"mixed-line {label}: setup {time.perf_counter() - t0:.2f} s, {mg.n_levels} levels, level-0 layout "
          f"{mg.level_layout(0)}, cyclic axes per level {[mg.line_cyclic(l) for l in range(mg.n_levels)]}", flush=True)
    z = torch.empty_like(b)
    calls = {"double": (mg.pcg, mg.apply_dev, mg.cycle_must_move()), "mixed": (mg.pcg_mixed, mg.apply_f32, mg.f32_must_move())}
    for name in calls:  # first calls: work vectors, float copies, captured graphs
        calls[name][1](b.data_ptr(), z.data_ptr())
    mg.sync()
    best = {}
    for rep_ in range(reps):
        for name, (solve, apply, mm) in calls.items():
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            _, it, rel = solve(rtol=rtol, max_iters=300)
            dt = time.perf_counter() - t0
            if name == "double":
                mg.zero_vec(0, "u")
                mg.sync()
            t0 = time.perf_counter()
            if name == "double":
                mg.vcycle(applies)
            else:
                for _ in range(applies):
                    apply(b.data_ptr(), z.data_ptr())
            mg.sync()
            da = (time.perf_counter() - t0) / applies
            old = best.get(name, (it, dt, da))
            best[name] = (it, min(old[1], dt), min(old[2], da))
            print(f"mixed-line {label}, {name} rep {rep_}: {it} iterations, {dt * 1e3:.2f} ms to {rtol:g} (relres "
                  f"{rel:.2e}, {'reached' if rel <= rtol else 'NOT reached'}), {da * 1e3:.3f} ms per application, "
                  f"must-move {mm / 1e6:.1f} MB = {mm / da / 8e12 * 100:.1f} % of 8 TB/s", flush=True)
    d, m = best["double"], best["mixed"]
    print(f"mixed-line {label} ({b.numel()} dofs): best solve double {d[0]} iterations {d[1] * 1e3:.2f} ms, mixed "
          f"{m[0]} iterations {m[1] * 1e3:.2f} ms, ratio {d[1] / m[1]:.2f}; best application double {d[2] * 1e3:.3f} ms, "
          f"mixed {m[2] * 1e3:.3f} ms, ratio {d[2] / m[2]:.2f}", flush=True)
    mg.close()


def mixed_line_cases(which=None):
    """profiles/mixed_line_config_bench.txt: the split-anisotropy operator through tensor_dev at 4096 x 1024
    and 256^3, and the periodic cyclic-lines operator of `periodic-lines` at the same sizes."""
    kw = dict(layout=amg.LAYOUT_SELL, **ALT_KW["alt 1+1"])

    def split(dims, L):
        def make():
            crow, col, val, b = torch_split_anisotropy_nd(dims)
            return amg.Multigrid.tensor_dev(crow, col, val, b, dims, L, **kw), b
        return make

    def cyclic(dims, eps, L):
        def make():
            crow, col, val, b = torch_scaled_periodic(dims, eps, 1)
            return amg.Multigrid.tensor_periodic_dev(crow, col, val, b, dims, L, 1, cyclic_lines=1, **kw), b
        return make
    cases = {"split2": ("4096 x 1024 split-anisotropy 1e-3", split((4096, 1024), 9)),
             "split3": ("256^3 split-anisotropy 1e-3", split((256, 256, 256), 7)),
             "cyclic2": ("4096 x 1024 x periodic, cyclic lines", cyclic((4096, 1024), (1.0, 1e-2), 9)),
             "cyclic3": ("256^3 x periodic, cyclic lines", cyclic((256, 256, 256), (1.0, 1e-2, 1e-2), 7))}
    for key, (label, make) in cases.items():
        if which in (None, key):
            run_mixed_line(label, make)


def run_mixed_dict(label, make, reps=3, rtol=1e-8, applies=10, by_level=False):
    """Three runs alternating in one process, best of `reps`, PCG to `rtol` from x = 0: amg_hip_pcg on the
    default (dictionary) layout, amg_hip_pcg_mixed on a layout = SELL solver, amg_hip_pcg_mixed on the
    dictionary solver (amg_hip_set_f32_dict).  Per run: iterations, wall ms, ms per preconditioner
    application over `applies` calls closed by one synchronise (double: vcycle(), the cycle amg_hip_pcg
    runs), and the must-move bytes of one application over that time as a share of 8 TB/s.  Then the level-0
    Jacobi sweep of the float dictionary kernel in its two rows-per-lane forms (amg_hip_set_dict_rows), and
    with by_level the float cycle's steps per level on both layouts."""
    import torch
    t0 = time.perf_counter()
    mg = make()
    sell = make(layout=amg.LAYOUT_SELL)
    mg.sync()
    nl = mg.n_levels
    lay = [mg.level_layout(l)[0] for l in range(nl - 1)]
    print(f"mixed-dict {label}: setup of both solvers {time.perf_counter() - t0:.2f} s, {nl} levels, layouts "
          f"{lay} (3 = dictionary) / SELL solver {[sell.level_layout(l)[0] for l in range(nl - 1)]}", flush=True)
    n = mg.get_n_dofs(0)
    b = torch.from_numpy(mg.get_rhs(0)).cuda()
    z = torch.empty_like(b)
    amg.set_f32_dict(1)
    runs = {"double dict": (mg, mg.pcg, None, mg.cycle_must_move()),
            "float SELL": (sell, sell.pcg_mixed, sell.apply_f32, sell.f32_must_move()),
            "float dict": (mg, mg.pcg_mixed, mg.apply_f32, mg.f32_must_move())}
    mg.apply_dev(b.data_ptr(), z.data_ptr())  # first calls: work vectors, float copies, captured graphs
    for name in ("float SELL", "float dict"):
        runs[name][2](b.data_ptr(), z.data_ptr())
    mg.sync()
    sell.sync()
    best = {}
    for rep_ in range(reps):
        for name, (m, solve, apply, mm) in runs.items():
            m.zero_vec(0, "u")
            m.sync()
            t0 = time.perf_counter()
            _, it, rel = solve(rtol=rtol, max_iters=300)
            dt = time.perf_counter() - t0
            m.zero_vec(0, "u")
            m.sync()
            t0 = time.perf_counter()
            if apply is None:
                m.vcycle(applies)
            else:
                for _ in range(applies):
                    apply(b.data_ptr(), z.data_ptr())
            m.sync()
            da = (time.perf_counter() - t0) / applies
            old = best.get(name, (it, dt, da))
            best[name] = (it, min(old[1], dt), min(old[2], da))
            print(f"mixed-dict {label}, {name} rep {rep_}: {it} iterations, {dt * 1e3:.2f} ms to {rtol:g} (relres "
                  f"{rel:.2e}, {'reached' if rel <= rtol else 'NOT reached'}), {da * 1e3:.3f} ms per application, "
                  f"must-move {mm / 1e6:.1f} MB = {mm / da / 8e12 * 100:.1f} % of 8 TB/s", flush=True)
    d, s, f = best["double dict"], best["float SELL"], best["float dict"]
    print(f"mixed-dict {label} ({n} dofs): best solve double dict {d[0]} it {d[1] * 1e3:.2f} ms, float SELL {s[0]} it "
          f"{s[1] * 1e3:.2f} ms, float dict {f[0]} it {f[1] * 1e3:.2f} ms (double / float dict {d[1] / f[1]:.2f}, float "
          f"SELL / float dict {s[1] / f[1]:.2f}); best application double dict {d[2] * 1e3:.3f} ms, float SELL "
          f"{s[2] * 1e3:.3f} ms, float dict {f[2] * 1e3:.3f} ms (double / float dict {d[2] / f[2]:.2f}, float SELL / "
          f"float dict {s[2] / f[2]:.2f})", flush=True)

    def op_us(m, l, op, count=20):
        m.f32_level_op(l, op)
        m.sync()
        t0 = time.perf_counter()
        for _ in range(count):
            m.f32_level_op(l, op)
        m.sync()
        return (time.perf_counter() - t0) / count * 1e6

    if mg.level_layout(0)[0] == amg.LAYOUT_DICT:
        # kernels.hip: DICT_F32_ROWS = 2 is the default form, amg_hip_set_dict_rows(1) selects the other
        launches = 2  # two Jacobi sweeps, or the two steps of Chebyshev(2)
        forms = {}
        for rep_ in range(reps):
            for rows, arg in ((2, 2), (4, 1)):
                amg.set_dict_rows(arg)
                us = op_us(mg, 0, 0) / launches
                forms[rows] = min(forms.get(rows, us), us)
        amg.set_dict_rows(2)
        stream = mg.level_layout(0)[1] + 12 * n  # the matrix stream (4 bytes per pair too many: < 1 KB) and x, f, out
        print(f"mixed-dict {label}: level-0 sweep of dict_f32_kernel, best of {reps} x 20 smoothings of 2 launches: "
              + ", ".join(f"{r} rows per lane {forms[r]:.1f} us ({stream / forms[r] / 8e6 * 100:.1f} % of 8 TB/s)"
                          for r in (2, 4)), flush=True)
    if by_level:
        for l in range(nl - 1):
            row = []
            for op, what in ((0, "smoothing"), (1, "residual"), (2, "restriction"), (3, "prolongation")):
                row.append(f"{what} {op_us(mg, l, op, 10):.1f} / {op_us(sell, l, op, 10):.1f}")
            print(f"mixed-dict {label}: level {l} ({mg.get_n_dofs(l)} rows, layout {mg.level_layout(l)[0]}) us per step, "
                  "float dict / float SELL: " + ", ".join(row), flush=True)
    amg.set_f32_dict(0)
    mg.close()
    sell.close()


def mixed_dict_cases(which=None):
    """profiles/mixed_dict_config_bench.txt"""
    jac = dict(smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.8)
    cheb = dict(smoother=amg.SM_CHEBYSHEV, smoother_iters=1, cheb_degree=2)

    def tensor(n, L, dim, opts):
        return lambda **kw: amg.Multigrid.poisson_tensor(n, L, dim=dim, device_setup=True, **dict(opts, **kw))

    def flat(**kw):
        return amg.Multigrid.poisson(4096, 16, **dict(KW["jacobi"], **kw))
    cases = {"t2": ("poisson_tensor 4096^2 / 10, Jacobi 0.8 2+2", tensor(4096, 10, 2, jac), True),
             "t3": ("poisson_tensor 256^3 / 7, Jacobi 0.8 2+2", tensor(256, 7, 3, jac), True),
             "c2": ("poisson_tensor 4096^2 / 10, Chebyshev(2) 1+1", tensor(4096, 10, 2, cheb), False),
             "flat": ("poisson 4096^2 / 16 (flat index), Jacobi 0.6 2+2", flat, False)}
    for key, (label, make, by_level) in cases.items():
        if which in (None, key):
            run_mixed_dict(label, make, by_level=by_level)


def block_memory(mg, kp, cheb):
    """device bytes the block cycle adds for pitch kp: per-level panels (U, F, R, T and Chebyshev D;
    U, F on the coarsest level), the coarse solve's three column buffers, and the CSR copies of the
    levels whose single-vector layout is not CSR (bounded by the structural nnz)"""
    L = mg.n_levels
    panels = 0
    csr = 0
    for l in range(L):
        n = mg.get_n_dofs(l)
        coarsest = l == L - 1 and l > 0
        panels += 8 * n * kp * (2 if coarsest else (5 if cheb else 4))
        if not coarsest and mg.level_layout(l)[0] != amg.LAYOUT_CSR:
            csr += 12 * amg.lib().amg_hip_get_level_nnz(mg._h, l) + 4 * (n + 1)
    panels += 3 * 8 * mg.get_n_dofs(L - 1) * kp
    return panels, csr


def run_block(label, mk, cycles=10, reps=3, ks=(1, 2, 4, 8, 16)):
    """ms per block cycle and right-hand-side cycles per second for k = 1..16, next to the single
    path's rate measured in the same run, alternating with it; the block cycle's must-move bytes
    per second as a fraction of 8 TB/s."""
    import numpy as np
    import torch
    mg = mk()
    mg.sync()
    n0 = mg.get_n_dofs(0)
    rng = np.random.default_rng(1)
    cheb = "cheb" in label
    print(f"{label}: {mg.n_levels} levels, {n0} dofs, coarse solve {mg.coarse_solve_kind().split(' ')[0]}",
          flush=True)
    for k in ks:
        U = torch.from_numpy(rng.standard_normal((n0, k))).cuda()
        F = torch.from_numpy(rng.standard_normal((n0, k))).cuda()
        mg.block_vcycles(U, F, n=2)   # CSR copies, panels, captured graph
        mg.vcycle(2)
        torch.cuda.synchronize()
        tb, ts = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            mg.block_vcycles(U, F, n=cycles)
            torch.cuda.synchronize()
            tb.append((time.perf_counter() - t0) / cycles)
            t0 = time.perf_counter()
            mg.vcycle(cycles)
            mg.sync()
            ts.append((time.perf_counter() - t0) / cycles)
        b, sgl = min(tb), min(ts)
        mm = mg.block_must_move(k)
        kp = 1 << (k - 1).bit_length()
        panels, csr = block_memory(mg, kp, cheb)
        print(f"  k={k:2d}: {b*1e3:8.3f} ms/block cycle = {k/b:9.1f} RHS-cycles/s | single {sgl*1e3:8.3f} ms = "
              f"{1/sgl:8.1f} cycles/s | block/single {(k/b)*sgl:5.2f}x | must-move {mm/1e6:9.1f} MB = "
              f"{mm/b/8e12*100:5.1f} % of 8 TB/s | block memory {panels/2**30:.2f} GiB panels + "
              f"{csr/2**30:.2f} GiB CSR copies", flush=True)
        del U, F
    mg.close()


def run_block_line(label, make, cycles=4, reps=3, ks=(1, 2, 4, 8, 16), rtol=1e-8, pcg=True):
    """A line-smoother solver made by make() (-> solver, level-0 right-hand side on the GPU) through the block
    entry points (amg_hip_set_block_lines) and through the single-vector path, alternating in one run, best of
    `reps`, per k: right-hand-side cycles per second (block_vcycles against vcycle) and right-hand-side solves
    per second to `rtol` by PCG from x = 0 (block_pcg on k copies of b scaled by 1 .. k against pcg on b), the
    block cycle's must-move bytes over its time as a share of 8 TB/s."""
    import torch
    t0 = time.perf_counter()
    mg, b = make()
    mg.sync()
    n0 = mg.get_n_dofs(0)
    print(f"block-line {label}: setup {time.perf_counter() - t0:.2f} s, {mg.n_levels} levels, {n0} dofs, level-0 "
          f"layout {mg.level_layout(0)}", flush=True)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for k in ks:
        U = torch.randn((n0, k), generator=g, device="cuda", dtype=torch.float64)
        F = torch.randn((n0, k), generator=g, device="cuda", dtype=torch.float64)
        B = (b[:, None] * torch.arange(1, k + 1, device="cuda", dtype=torch.float64)[None, :]).contiguous()
        X = torch.zeros_like(B)
        mg.block_vcycles(U, F, n=2)   # CSR copies, panels, captured graph
        mg.vcycle(2)
        torch.cuda.synchronize()
        tb, ts, pb, ps = [], [], [], []
        itb = its = relb = rels = None
        for _ in range(reps):
            t0 = time.perf_counter()
            mg.block_vcycles(U, F, n=cycles)
            torch.cuda.synchronize()
            tb.append((time.perf_counter() - t0) / cycles)
            t0 = time.perf_counter()
            mg.vcycle(cycles)
            mg.sync()
            ts.append((time.perf_counter() - t0) / cycles)
            if not pcg:
                continue
            X.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, itb, relb = mg.block_pcg(B, X, rtol=rtol, max_iters=300)
            torch.cuda.synchronize()
            pb.append(time.perf_counter() - t0)
            mg.copy_vec_dev(0, "f", b.data_ptr(), to_solver=True)
            mg.zero_vec(0, "u")
            mg.sync()
            t0 = time.perf_counter()
            it1, rel1 = ctypes.c_int64(0), ctypes.c_double(0)   # amg_hip_pcg itself: the solution stays on the device
            assert amg.lib().amg_hip_pcg(mg._h, rtol, 300, ctypes.byref(it1), ctypes.byref(rel1)) == 0
            mg.sync()
            ps.append(time.perf_counter() - t0)
            its, rels = it1.value, rel1.value
        blk, sgl = min(tb), min(ts)
        mm = mg.block_must_move(k)
        line = (f"  k={k:2d}: {blk*1e3:8.3f} ms/block cycle = {k/blk:8.1f} RHS-cycles/s | single {sgl*1e3:8.3f} ms = "
                f"{1/sgl:7.1f} cycles/s | block/single {(k/blk)*sgl:5.2f}x | must-move {mm/1e6:9.1f} MB = "
                f"{mm/blk/8e12*100:5.1f} % of 8 TB/s")
        if pcg:
            line += (f" | PCG to {rtol:g}: block {max(itb)} iterations {min(pb)*1e3:8.2f} ms = {k/min(pb):7.1f} RHS-solves/s"
                     f" (worst relres {max(relb):.1e}) | single {its} iterations {min(ps)*1e3:8.2f} ms = "
                     f"{1/min(ps):6.1f} solves/s (relres {rels:.1e}) | block/single {(k/min(pb))*min(ps):5.2f}x")
        print(line, flush=True)
        del U, F, B, X
    mg.close()


def block_line_cases(which=None, **kw):
    """profiles/block_line_config_bench.txt: AMG_HIP_SM_LINE_JACOBI 1+1 omega 0.7 on poisson(4096, 16);
    AMG_HIP_SM_LINE_ALT 1+1 omega 0.8 on the split-anisotropy operator (1e-3) at 4096 x 1024 / 9 levels and
    256^3 / 7 levels; the 4096 x 1024 cyclic-lines operator of `periodic-lines` (x periodic)."""
    import torch
    alt = ALT_KW["alt 1+1"]

    def poisson():
        mg = amg.Multigrid.poisson(4096, 16, **KW["line"])
        b = torch.empty(mg.get_n_dofs(0), dtype=torch.float64, device="cuda")
        mg.copy_vec_dev(0, "f", b.data_ptr(), to_solver=False)
        mg.sync()
        return mg, b

    def split(dims, L):
        def make():
            crow, col, val, b = torch_split_anisotropy_nd(dims)
            return amg.Multigrid.tensor_dev(crow, col, val, b, dims, L, **alt), b
        return make

    def cyclic(dims, eps, L):
        def make():
            crow, col, val, b = torch_scaled_periodic(dims, eps, 1)
            return amg.Multigrid.tensor_periodic_dev(crow, col, val, b, dims, L, 1, cyclic_lines=1, **alt), b
        return make
    cases = {"jacobi": ("poisson(4096, 16) line Jacobi 1+1 omega 0.7", poisson),
             "split2": ("4096 x 1024 / 9 split-anisotropy 1e-3, alternating lines 1+1 omega 0.8", split((4096, 1024), 9)),
             "split3": ("256^3 / 7 split-anisotropy 1e-3, alternating lines 1+1 omega 0.8", split((256, 256, 256), 7)),
             "cyclic2": ("4096 x 1024 / 9 x periodic, cyclic lines, alternating lines 1+1 omega 0.8",
                         cyclic((4096, 1024), (1.0, 1e-2), 9))}
    for key, (label, make) in cases.items():
        if which in (None, key):
            run_block_line(label, make, **kw)


if len(sys.argv) > 1 and sys.argv[1].startswith("block"):
    import torch  # noqa: F401  (before the library: torch needs its own HIP runtime)
if len(sys.argv) > 1 and sys.argv[1] == "block-line":
    # profiles/block_line_config_bench.txt; an argument picks one case: jacobi | split2 | split3 | cyclic2
    amg.set_periodic_device_setup(1)
    amg.set_block_lines(1)
    block_line_cases(sys.argv[2] if len(sys.argv) > 2 else None)
elif len(sys.argv) > 2 and sys.argv[1] == "block-line8":   # one case at k = 8, cycles only (kernel traces)
    amg.set_periodic_device_setup(1)
    amg.set_block_lines(1)
    block_line_cases(sys.argv[2], reps=1, ks=(8,), pcg=False)
elif len(sys.argv) > 1 and sys.argv[1] == "block":
    def rs(sm):
        cp, ri, v = amg.laplacian(1024)
        return lambda: amg.Multigrid.ruge_stueben(cp, ri, v, amg.rhs(1024), 25, 0.25, 500, **KW[sm])
    run_block("RS 1024^2 jacobi 2+2", rs("jacobi"))
    run_block("RS 1024^2 cheb(2) 1+1", rs("cheb"))
    run_block("poisson(1024, 6) jacobi 2+2", lambda: amg.Multigrid.poisson(1024, 6, **KW["jacobi"]))
    run_block("poisson(4096, 16) jacobi 2+2", lambda: amg.Multigrid.poisson(4096, 16, **KW["jacobi"]), cycles=4)
    run_block("poisson(256, 17, dim=3) jacobi 2+2",
              lambda: amg.Multigrid.poisson(256, 17, dim=3, **KW["jacobi"]), cycles=4)
elif len(sys.argv) > 2 and sys.argv[1] == "block8":   # one workload at k = 8 (kernel traces): rs | p4096
    if sys.argv[2] == "rs":
        cp, ri, v = amg.laplacian(1024)
        run_block("RS 1024^2 jacobi 2+2", lambda: amg.Multigrid.ruge_stueben(cp, ri, v, amg.rhs(1024), 25, 0.25, 500,
                                                                          **KW["jacobi"]), reps=1, ks=(8,))
    else:
        run_block("poisson(4096, 16) jacobi 2+2", lambda: amg.Multigrid.poisson(4096, 16, **KW["jacobi"]), cycles=4,
                  reps=1, ks=(8,))
elif len(sys.argv) > 1 and sys.argv[1] == "tensor":
    run_tensor(4096, 10, 16)                           # the bench.py problem; coarsest 8 x 8
    run_tensor(1024, 8, 12)
elif len(sys.argv) > 1 and sys.argv[1] == "tensor-setup":
    os.environ.setdefault("AMG_HIP_TIMING", "1")
    if len(sys.argv) > 4:
        run_tensor_setup(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        run_tensor_setup(2, 1024, 8)
        run_tensor_setup(2, 4096, 10)
        run_tensor_setup(3, 256, 7)
elif len(sys.argv) > 1 and sys.argv[1] == "tensor-user-setup":
    os.environ.setdefault("AMG_HIP_TIMING", "1")
    import torch  # noqa: F401  (before the library is loaded: INTEGRATION.md, section 2)
    if len(sys.argv) > 5:
        d = tuple(int(x) for x in sys.argv[2:5])
        run_tensor_user_setup(d if d[2] > 1 else d[:2], int(sys.argv[5]))
    else:
        run_tensor_user_setup((1024, 1024), 8)
        run_tensor_user_setup((4096, 4096), 10)
        run_tensor_user_setup((256, 256, 256), 7)
        run_tensor_user_setup((4096, 1024), 9)
elif len(sys.argv) > 1 and sys.argv[1] == "alt":
    import torch  # noqa: F401  (before the library is loaded: INTEGRATION.md, section 2)
    if len(sys.argv) > 4:
        run_alt((int(sys.argv[2]), int(sys.argv[3])), int(sys.argv[4]))
    else:
        run_alt((4096, 4096), 10)
        run_alt((4096, 1024), 9)
elif len(sys.argv) > 2 and sys.argv[1] == "alt10":     # ten cycles of the alternating smoother (kernel traces)
    import torch  # noqa: F401
    d = (int(sys.argv[2]), int(sys.argv[3]))
    mg = amg.Multigrid.tensor_dev(*torch_split_anisotropy(d), d, int(sys.argv[4]), **ALT_KW["alt 1+1"])
    mg.vcycle(2)
    mg.sync()
    mg.vcycle(10)
    mg.sync()
    mg.close()
elif len(sys.argv) > 1 and sys.argv[1] == "mixed":
    import torch  # noqa: F401  (before the library is loaded: INTEGRATION.md, section 2)
    if len(sys.argv) > 5:
        d = tuple(int(x) for x in sys.argv[2:5])
        run_mixed(d if d[2] > 1 else d[:2], int(sys.argv[5]))
    else:
        run_mixed((1024, 1024), 8)
        run_mixed((4096, 4096), 10)
        run_mixed((256, 256, 256), 7)
elif len(sys.argv) > 1 and sys.argv[1] == "semi":
    # profiles/semi_config_bench.txt: a 4096 x 1024 grid with a weak y axis, a 256^3 box with a weak z axis
    if len(sys.argv) > 7:
        d = tuple(int(x) for x in sys.argv[2:5])
        e = tuple(float(x) for x in sys.argv[5:8])
        run_semi(d if d[2] > 1 else d[:2], e if d[2] > 1 else e[:2])
    else:
        run_semi((4096, 1024), (1.0, 1e-2))
        run_semi((256, 256, 256), (1.0, 1.0, 1e-2))
elif len(sys.argv) > 1 and sys.argv[1] == "opdep":
    if len(sys.argv) > 4:
        d = tuple(int(x) for x in sys.argv[2:5])
        run_opdep(d if d[2] > 1 else d[:2])
    else:
        run_opdep((2048, 2048))
        run_opdep((128, 128, 128))
elif len(sys.argv) > 1 and sys.argv[1] == "opdep-periodic":
    # profiles/opdep_periodic_config_bench.txt
    if len(sys.argv) > 4:
        d = tuple(int(x) for x in sys.argv[2:5])
        run_opdep_periodic(d if d[2] > 1 else d[:2])
    else:
        run_opdep_periodic((2048, 2048))
        run_opdep_periodic((128, 128, 128))
elif len(sys.argv) > 1 and sys.argv[1] == "opdep-setup":
    # profiles/opdep_setup.txt
    os.environ.setdefault("AMG_HIP_TIMING", "1")
    import torch  # noqa: F401  (before the library is loaded: INTEGRATION.md, section 2)
    if len(sys.argv) > 4:
        d = tuple(int(x) for x in sys.argv[2:5])
        run_opdep_setup(d if d[2] > 1 else d[:2])
    else:
        run_opdep_setup((2048, 2048))
        run_opdep_setup((128, 128, 128))
elif len(sys.argv) > 1 and sys.argv[1] == "opdep-periodic-setup":
    # profiles/opdep_periodic_setup.txt
    os.environ.setdefault("AMG_HIP_TIMING", "1")
    import torch  # noqa: F401  (before the library is loaded: INTEGRATION.md, section 2)
    if len(sys.argv) > 4:
        d = tuple(int(x) for x in sys.argv[2:5])
        run_opdep_periodic_setup(d if d[2] > 1 else d[:2])
    else:
        run_opdep_periodic_setup((2048, 2048))
        run_opdep_periodic_setup((128, 128, 128))
elif len(sys.argv) > 4 and sys.argv[1] == "opdep10":    # ten cycles of one hierarchy (kernel traces)
    d = tuple(int(x) for x in sys.argv[2:5])
    d = d if d[2] > 1 else d[:2]
    mg = make_opdep(numpy_jump(d), d, csr=len(sys.argv) > 5)
    mg.vcycle(10)
    mg.sync()
    mg.close()
elif len(sys.argv) > 1 and sys.argv[1] == "natural":
    # profiles/natural_config_bench.txt
    if len(sys.argv) > 4:
        d = tuple(int(x) for x in sys.argv[2:5])
        run_natural(d if d[2] > 1 else d[:2])
    else:
        run_natural((4096, 1024))
        run_natural((256, 256, 256))
elif len(sys.argv) > 1 and sys.argv[1] == "singular":
    # profiles/singular_config_bench.txt
    if len(sys.argv) > 4:
        d = tuple(int(x) for x in sys.argv[2:5])
        run_singular(d if d[2] > 1 else d[:2])
    else:
        run_singular((4096, 1024))
        run_singular((256, 256, 256))
elif len(sys.argv) > 1 and sys.argv[1] == "periodic":
    # profiles/periodic_config_bench.txt
    if len(sys.argv) > 4:
        d = tuple(int(x) for x in sys.argv[2:5])
        run_periodic(d if d[2] > 1 else d[:2])
    else:
        run_periodic((4096, 1024))
        run_periodic((256, 256, 256))
elif len(sys.argv) > 1 and sys.argv[1] == "periodic-lines":
    # profiles/periodic_cyclic_config_bench.txt
    import torch  # noqa: F401  (before the library is loaded: INTEGRATION.md, section 2)
    amg.set_periodic_device_setup(1)  # the hierarchy on the device: the same solver, set up sooner
    run_periodic_lines((4096, 1024), (1.0, 1e-2), 9)
    run_periodic_lines((256, 256, 256), (1.0, 1e-2, 1e-2), 7)
elif len(sys.argv) > 1 and sys.argv[1] == "mixed-line":
    # profiles/mixed_line_config_bench.txt; an argument picks one case: split2 | split3 | cyclic2 | cyclic3
    import torch  # noqa: F401  (before the library is loaded: INTEGRATION.md, section 2)
    amg.set_periodic_device_setup(1)
    amg.set_f32_lines(1)
    mixed_line_cases(sys.argv[2] if len(sys.argv) > 2 else None)
elif len(sys.argv) > 1 and sys.argv[1] == "mixed-dict":
    # profiles/mixed_dict_config_bench.txt; an argument picks one case: t2 | t3 | c2 | flat
    import torch  # noqa: F401  (before the library is loaded: INTEGRATION.md, section 2)
    mixed_dict_cases(sys.argv[2] if len(sys.argv) > 2 else None)
elif len(sys.argv) > 1 and sys.argv[1] == "periodic-setup":
    # profiles/periodic_setup.txt
    os.environ.setdefault("AMG_HIP_TIMING", "1")
    import torch  # noqa: F401  (before the library is loaded: INTEGRATION.md, section 2)
    if len(sys.argv) > 4:
        d = tuple(int(x) for x in sys.argv[2:5])
        run_periodic_setup(d if d[2] > 1 else d[:2])
    else:
        run_periodic_setup((1024, 1024))
        run_periodic_setup((4096, 1024))
        run_periodic_setup((256, 256, 256))
elif len(sys.argv) > 3 and sys.argv[1] == "tensor10":
    mg = amg.Multigrid.poisson_tensor(int(sys.argv[2]), int(sys.argv[3]), stencil_transfers=len(sys.argv) < 5,
                                      **TENSOR_KW["jacobi"])
    mg.vcycle(5)                                       # warm-up
    mg.sync()
    mg.vcycle(10)
    mg.sync()
    mg.close()
elif len(sys.argv) > 1 and sys.argv[1] == "cheb":
    run(2, 4096, 16, "cheb", 20)                       # the bench.py problem, Chebyshev(2) 1+1
    run(2, 4096, 16, "jacobi", 20)                     # ... next to true Jacobi 2+2
    run_rs(1024, "cheb")                               # RS 1024^2: rate, 1e-8, PCG to 1e-8
    run_rs(1024, "cheb3")
    run_rs(1024, "jacobi")
    run(3, 256, 17, "cheb", 10)                        # 256^3 3-D
    run(3, 256, 17, "jacobi", 10)
elif len(sys.argv) > 1 and sys.argv[1] == "line":
    run_to_tol(2, 4096, 16, pcg_levels=9)              # the bench.py problem: line 1+1 next to true Jacobi 2+2
    run_to_tol(2, 1024, 12)
    run_to_tol(3, 256, 17, cap=200, reps=1)            # 3-D: no gain expected (a line covers one of two directions)
elif len(sys.argv) > 2 and sys.argv[1] == "line10":    # ten cycles of one smoother at 4096^2 (kernel traces)
    run(2, 4096, 16, sys.argv[2], 10, warm=2)
elif len(sys.argv) > 1 and sys.argv[1] == "rs":
    for n in (512, 1024, 2048):
        run_rs(n, "multicolor")
        run_rs(n, "jacobi")
    run_rs(1024, "spgs", 5)
    run_rs(64, "jacobi", 10, dim=3)
elif len(sys.argv) > 1 and sys.argv[1] == "all":
    run(2, 128, 3, "spgs", 20)                         # BASELINE config 1 (exact kernel: small)
    run(2, 1024, 6, "spgs", 5)                         # config 2, the reference's default smoother
    run(2, 1024, 6, "spgs", 5, exact_gs=True, exact_coarse_solve=True)   # ... parity mode
    run(2, 1024, 6, "jacobi1", 20)                     # config 2, true Jacobi 1+1
    run(2, 1024, 6, "jacobi1", 20, exact_coarse_solve=True)
    run(2, 1024, 12, "jacobi", 20)
    run(2, 1024, 6, "multicolor", 10)
    run(2, 4096, 16, "jacobi", 20)                     # config 3 (bench.py headline)
    run(2, 4096, 9, "jacobi", 20)
    run(2, 4096, 16, "multicolor", 10)
    run(2, 8192, 18, "jacobi", 10)                     # config 4 grid
    run(2, 8192, 9, "jacobi", 10)
    run(2, 8192, 18, "multicolor", 10)                 # config 4
    run(2, 8192, 9, "multicolor", 10)
    run(3, 256, 17, "jacobi", 10)
    run(3, 512, 20, "jacobi", 10)                      # config 5 grid on ONE GPU
else:
    dim, n, L, sm = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    run(dim, n, L, sm, int(sys.argv[5]) if len(sys.argv) > 5 else 10)
