#!/usr/bin/env python3
"""DIAGNOSTIC (GPU box): phase shares, residency and dispatch gaps of a K-Patch down-leg from the
stamps of a -DAMG_PATCH_STAMPS build (kernels.hip: patch_stamp), for the whole launch and split by
the tile's flag (one type / column-typed / general).  Never a timing source.
usage: AMG_HIP_LIBRARY=<stamps build> python tools/patch_stamps.py [n [level ...]]
The leg of each level is the one a whole V-cycle launches (the stamps are filtered by the level's rows)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "algebraic-multigrid_amd"))
import amg_ctypes as amg  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
levels = [int(a) for a in sys.argv[2:]] or [0]
lib = amg.lib()
L = 16 if n == 4096 else 12
mg = amg.Multigrid.poisson(n, L, smoother=amg.SM_JACOBI, smoother_iters=2, omega=0.6)
mg.vcycle(3)
mg.sync()
dbg = C.CDLL(os.environ.get("AMG_HIP_LIBRARY", amg.LIB_PATH))
fn = dbg.amg_hip_debug_patch_stamps
fn.argtypes = [C.c_void_p]
fn_rows = dbg.amg_hip_debug_patch_stamps_rows
fn_rows.argtypes = [C.c_int32]
NAMES = ["load (entry -> tile in LDS)", "sweep 1", "sweep 2", "copy-out + residual", "restriction + coarse sweep"]


def by_flag(s, t, dur, m):
    """workgroup life and phase shares by the flag the kernel read for its tile (stamp slot 6)"""
    tf = (s[:, 6] & 255).astype(np.int64)
    ftile = (s[:, 6] >> 8).astype(np.int64)
    pxc = m // 64
    px, py = ftile % pxc, ftile // pxc
    edge_col = (px == 0) | (px == pxc - 1)
    edge_row = (py == 0) | (py == py.max())
    classes = [("one type (flag < 254)", tf < 254), ("column-typed (flag 254)", tf == 254), ("general (flag 255)", tf == 255),
               ("  general, edge column, inner tile row", (tf == 255) & edge_col & ~edge_row),
               ("  general, top / bottom tile row", (tf == 255) & edge_row),
               ("  general, elsewhere", (tf == 255) & ~edge_col & ~edge_row)]
    med = {}
    for name, sel in classes:
        k = int(sel.sum())
        if k == 0:
            print(f"  {name:42s} 0 workgroups")
            continue
        d = dur[sel]
        med[name] = float(np.median(d))
        sh = " / ".join(f"{100 * (t[sel, q + 1] - t[sel, q]).mean() / d.mean():4.1f}" for q in range(5))
        print(f"  {name:42s} {k:5d} workgroups ({100 * k / len(dur):4.1f} %), life median {np.median(d):6.2f} us  mean {d.mean():6.2f}  "
              f"p10 {np.percentile(d, 10):6.2f}  p90 {np.percentile(d, 90):6.2f}; shares load/sw1/sw2/resid/restr {sh} %")
    a, b = med.get("  general, edge column, inner tile row"), med.get("one type (flag < 254)")
    if a and b:
        print(f"  edge-column general tiles live {a / b:.2f} x as long as one-type tiles (medians)")
    a = med.get("column-typed (flag 254)")
    if a and b:
        print(f"  column-typed tiles live {a / b:.2f} x as long as one-type tiles (medians)")
    # which class the launch waits for: the last workgroups to end
    order = np.argsort(t[:, 5])[::-1][:max(1, len(dur) // 20)]
    print(f"  of the last 5 % of workgroups to end: {100 * np.mean(tf[order] == 255):.0f} % general, "
          f"{100 * np.mean(tf[order] == 254):.0f} % column-typed, {100 * np.mean(tf[order] < 254):.0f} % one type")


def report(level):
    m = n >> level                    # pitch of the level's band; the level has n lines of m rows
    rows = mg.get_n_dofs(level)
    th = mg.patch_leg_lines(level, 0)
    assert th > 0 and m >= 128, f"level {level} ({rows} rows) is no K-Patch level"
    tiles = (((rows + m - 1) // m + th - 1) // th) * (m // 64)
    cap = ((n + 37) // 38) * (m // 64)  # the shortest tiles any leg uses: room for every workgroup, whatever ran
    buf = torch.zeros(cap * 8, dtype=torch.int64, device="cuda")
    assert fn_rows(rows) == 0
    assert fn(C.c_void_p(buf.data_ptr())) == 0
    mg.vcycle(1)                      # whole cycles: the level's down-leg in its place; the last one's stamps stay
    mg.vcycle(1)
    mg.sync()
    fn(C.c_void_p(0))
    s = buf.cpu().numpy().reshape(cap, 8)
    got = int((s[:, 5] != 0).sum())
    if got != tiles or not (s[:tiles, 5] != 0).all():
        print(f"== level {level}: {got} workgroups left stamps, the leg of {rows} rows should have {tiles}; "
              f"rows by level: {[mg.get_n_dofs(q) for q in range(min(6, mg.n_levels()))]}")
        return
    s = s[:tiles]
    print(f"== level {level} down-leg ({rows} rows, pitch {m}, tiles of {th} lines)")
    analyse(s, tiles, m)


def analyse(s, tiles, m):
    t = s[:, :6].astype(np.float64) * 0.01      # us (100 MHz)
    t0 = t[:, 0].min()
    t -= t0
    dur = t[:, 5] - t[:, 0]
    print(f"{tiles} workgroups, kernel span {t[:, 5].max():.1f} us (diagnostic build), workgroup life avg {dur.mean():.2f} us "
          f"(min {dur.min():.2f}, max {dur.max():.2f})")
    for k in range(5):
        d = t[:, k + 1] - t[:, k]
        print(f"  {NAMES[k]:32s} avg {d.mean():6.2f} us  p10 {np.percentile(d, 10):6.2f}  p90 {np.percentile(d, 90):6.2f}  share {100 * d.mean() / dur.mean():5.1f} %")
    hw = s[:, 7]
    xcc = (hw >> 32) & 0xF
    cu = (hw >> 8) & 0xF
    sh = (hw >> 12) & 1
    se = (hw >> 13) & 7
    key = ((xcc * 8 + se) * 2 + sh) * 16 + cu
    cus = np.unique(key)
    print(f"distinct CUs seen: {cus.size}")
    # residency: time-average number of workgroups alive per CU; gaps between an end and the next start on that CU
    span = t[:, 5].max()
    alive = dur.sum() / (cus.size * span)
    print(f"time-average workgroups resident per CU: {alive:.2f}")
    gaps, conc = [], []
    for c in cus:
        idx = np.nonzero(key == c)[0]
        ev = sorted([(t[i, 0], 1) for i in idx] + [(t[i, 5], -1) for i in idx])
        cur, mx = 0, 0
        for _, d in ev:
            cur += d
            mx = max(mx, cur)
        conc.append(mx)
    print(f"max concurrent workgroups on a CU: min {min(conc)}, median {int(np.median(conc))}, max {max(conc)}; workgroups per CU: "
          f"min {min(np.sum(key == c) for c in cus)}, max {max(np.sum(key == c) for c in cus)}")
    # slots idle while work was still waiting: per CU, integrate (4 - resident) until the CU's last start
    idle, busy = 0.0, 0.0
    for c in cus:
        idx = np.nonzero(key == c)[0]
        last_start = t[idx, 0].max()
        ev = sorted([(t[i, 0], 1) for i in idx] + [(t[i, 5], -1) for i in idx])
        cur, prev = 0, 0.0
        for tm, d in ev:
            if tm > last_start:
                tm = last_start
            idle += (4 - cur) * max(0.0, tm - prev)
            busy += cur * max(0.0, tm - prev)
            prev = max(prev, tm)
            cur += d
    print(f"before a CU's last workgroup starts: {100 * idle / (idle + busy):.1f} % of its four slots stand empty")
    # gap between a workgroup's end and the next start on the same CU
    g = []
    for c in cus:
        idx = np.nonzero(key == c)[0]
        st = np.sort(t[idx, 0])
        en = np.sort(t[idx, 5])
        for e in en:
            nxt = st[st >= e]
            if nxt.size:
                g.append(nxt[0] - e)
    g = np.array(g)
    if g.size:
        print(f"end -> next start on the same CU: median {np.median(g):.2f} us, p90 {np.percentile(g, 90):.2f} us")
    starts = np.sort(t[:, 0])
    print("start times (us) percentiles 0/25/50/75/100:", [round(float(np.percentile(starts, q)), 1) for q in (0, 25, 50, 75, 100)])
    ends = np.sort(t[:, 5])
    print("end times   (us) percentiles 0/25/50/75/100:", [round(float(np.percentile(ends, q)), 1) for q in (0, 25, 50, 75, 100)])
    # per-XCD finish
    for x in range(8):
        on = xcc == x
        if on.any():
            print(f"  XCD {x}: {int(on.sum())} workgroups, last end {t[on, 5].max():.1f} us, CUs {np.unique(key[on]).size}")
    print("by tile flag:")
    by_flag(s, t, dur, m)


for lv in levels:
    report(lv)
