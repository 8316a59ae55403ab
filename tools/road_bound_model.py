"""CPU model of lidar_body's road march (statistics only, not a parity tool; the
shipped bounds are checked by tests/native/roadbound_check.cpp): queued beams and
phase-2 iterations for variants of the road/screen safe-distance bound, on poses
from the C oracle stepping uniform random actions with auto-reset (the bench
workload).  The march is the kernel's: a jump of 1 + safe_steps from the car
centre, LIDAR_NPR probes (phase 1), then iterations of 2 probes and a jump.
    python tools/road_bound_model.py [--envs 64] [--steps 200]"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

f32 = np.float32
W = 750


def poses(envs, steps, n=8, rays=64, seed=0):
    from oracle.oracle import OracleEnv
    rng = np.random.default_rng(seed)
    out = []
    for e in range(envs):
        env = OracleEnv(n_agents=n, rays=rays, use_team=True)
        P = env.P
        env.reset(rng.integers(0, 12, n))  # route ids of the default 3-lane layout
        for t in range(steps):
            r = env.step(rng.uniform(-1, 1, (n, 2)).astype(np.float32))
            if r["terminated"] or r["truncated"]:
                env.reset(rng.integers(0, 12, n))
            if t % 10 == 9:
                eg, _, _ = env.get_state()
                for i in range(n):
                    if eg["alive"][i]:
                        out.append((eg["x"][i], eg["y"][i], eg["h"][i]))
        env.close()
    return np.array(out, np.float32)


def safe_v0(fx, fy, dx, dy, rw):
    """The current device bound (road_safe in mev_roadbound.h)."""
    ccen, crf = f32(rw + 84), f32(84)
    rwm = f32(rw - 1.5)
    idx, idy = f32(1) / dx, f32(1) / dy
    iadx, iady = np.abs(idx), np.abs(idy)
    rx, ry = fx - f32(375), fy - f32(375)
    ax, ay = np.abs(rx), np.abs(ry)
    sx = np.where(ax < rwm, rwm * iadx - rx * idx, 0)
    sy = np.where(ay < rwm, rwm * iady - ry * idy, 0)
    sqm, rg = ccen - f32(1.55), crf + f32(2)
    ocx = rx - np.where(np.where(rx != 0, rx, dx) >= 0, ccen, -ccen)
    ocy = ry - np.where(np.where(ry != 0, ry, dy) >= 0, ccen, -ccen)
    return _rest(fx, fy, dx, dy, idx, idy, iadx, iady, rx, ry, ax, ay, sx, sy, sqm, rg, ocx, ocy, f32(0.5), f32(748.5))


def safe_v1(fx, fy, dx, dy, rw, strip_half=None):
    """Per-axis exact intervals about 375.5 (truncation = floor on screen): strips
    hold pixels |p - 375| <= rw - 1 (the tangent pixels of the grass discs sit at
    |p - 375| = rw), the square |p - 375| <= rw + cr, the disc grown by sqrt(2)/2
    about the pixel-offset centre, the screen [0, 750)."""
    eps = f32(0.01)
    ccen, crf = f32(rw + 84), f32(84)
    rwm = f32(rw - 0.5) - eps if strip_half is None else f32(strip_half)
    idx, idy = f32(1) / dx, f32(1) / dy
    iadx, iady = np.abs(idx), np.abs(idy)
    rx, ry = fx - f32(375.5), fy - f32(375.5)
    ax, ay = np.abs(rx), np.abs(ry)
    sx = np.where(ax < rwm, rwm * iadx - rx * idx, 0)
    sy = np.where(ay < rwm, rwm * iady - ry * idy, 0)
    sqm, rg = ccen + f32(0.5) - eps, crf + f32(0.7072) + eps
    ocx = rx - np.where(np.where(rx != 0, rx, dx) >= 0, ccen, -ccen)
    ocy = ry - np.where(np.where(ry != 0, ry, dy) >= 0, ccen, -ccen)
    return _rest(fx, fy, dx, dy, idx, idy, iadx, iady, rx, ry, ax, ay, sx, sy, sqm, rg, ocx, ocy, eps, f32(750) - eps)


def _rest(fx, fy, dx, dy, idx, idy, iadx, iady, rx, ry, ax, ay, sx, sy, sqm, rg, ocx, ocy, slo, shi):
    big = f32(1e6)
    bq = ocx * dx + ocy * dy
    cq = ocx * ocx + ocy * ocy - rg * rg
    disc = bq * bq - cq
    with np.errstate(invalid="ignore"):
        root = -bq - np.sqrt(np.maximum(disc, 0))
    tdisc = np.where(cq <= 0, 0, np.where((disc < 0) | (bq >= 0), big, root))
    tsq = np.minimum(sqm * iadx - rx * idx, sqm * iady - ry * idy)
    tq = np.minimum(np.where(rx * dx < 0, -rx * idx, big), np.where(ry * dy < 0, -ry * idy, big))
    sc = np.where(np.maximum(ax, ay) < sqm, np.minimum(tdisc, np.minimum(tsq, tq)), 0)
    road = np.maximum(np.maximum(sx, sy), sc)
    tx = np.where(dx > 0, shi - fx, fx - slo) * iadx
    ty = np.where(dy > 0, shi - fy, fy - slo) * iady
    return np.minimum(road, np.minimum(tx, ty))


def safe_entry(fx, fy, dx, dy, rw):
    """road_entry_safe (mev_roadbound.h): the ray's first entry into the four grown grass quadrants."""
    never = f32(1e6)
    ccen, crf = f32(rw + 84), f32(84)
    rwm, sqm, rg = f32(rw - 1.5), ccen - f32(1.55), crf + f32(2)
    with np.errstate(all="ignore"):
        iadx, iady = np.abs(f32(1) / dx), np.abs(f32(1) / dy)
        rx, ry = fx - f32(375), fy - f32(375)
        x, y = np.where(dx < 0, -rx, rx), np.where(dy < 0, -ry, ry)
        a, b = np.abs(dx), np.abs(dy)
        txp, txm, txs = (rwm - x) * iadx, (-rwm - x) * iadx, (sqm - x) * iadx
        typ, tym, tys = (rwm - y) * iady, (-rwm - y) * iady, (sqm - y) * iady
        inx, iny = np.fmax(txp, 0), np.fmax(typ, 0)
        t1 = np.fmax(inx, iny)
        xn, yn = x < -rwm, y < -rwm
        v4, v2, v3 = xn & yn, xn & (iny < txm), yn & (inx < tym)
        mA = np.where(v2, iny, np.where(v3, inx, t1))
        oA = np.where(v2, txm, np.where(v3, tym, never))
        mB = np.where(v2 | v3, t1, never)
        m1, o1, m2 = np.where(v4, 0, mA), np.where(v4, np.fmin(txm, tym), oA), np.where(v4, mA, mB)
        xg, yg = ~(v4 | v2), ~(v4 | v3)
        ue, ve = np.abs(x + a * m1), np.abs(y + b * m1)
        ocx, ocy = ue - ccen, ve - ccen
        bq = ocx * np.where(xg, a, -a) + ocy * np.where(yg, b, -b)
        cq = ocx * ocx + ocy * ocy - rg * rg
        disc = bq * bq - cq
        root = -bq - np.sqrt(np.maximum(disc, 0))
        tdisc = np.where(cq <= 0, 0, np.where((disc < 0) | (bq >= 0), never, root))
        tcorner = np.fmin(m1 + tdisc, np.fmin(np.where(xg, txs, never), np.where(yg, tys, never)))
        tq = np.where(np.maximum(ue, ve) >= sqm, m1, np.where(tcorner < o1, tcorner, never))
        road = np.fmin(tq, m2)
        tx = (np.where(dx > 0, f32(373.5), f32(374.5)) - x) * iadx
        ty = (np.where(dy > 0, f32(373.5), f32(374.5)) - y) * iady
        return np.fmin(road, np.fmin(tx, ty)).astype(f32)


def on_road_px(px, py, rw):
    ccen, cr = rw + 84, 84
    iax, iay = np.abs(px - 375), np.abs(py - 375)
    qdx, qdy = iax - ccen, iay - ccen
    onv = np.maximum(np.minimum(np.minimum(iax, iay) - rw, np.maximum(iax, iay) - ccen), cr * cr + 1 - (qdx * qdx + qdy * qdy))
    return onv <= 0


NPR = 2  # LIDAR_NPR


def march(P, rel, safe1, safe2, pre=False, rw=126, stp=4.0, S=63):
    """lidar_body's march with phase 1's bound safe1 and phase 2's safe2 (pre: phase 2 jumps from the
    beam's last tested probe before its probes, else after them).  Returns (phase-2 iterations per
    beam, stop index per beam); a beam with 0 iterations finished in phase 1."""
    A, R = len(P), len(rel)
    cx = np.repeat(P[:, 0], R); cy = np.repeat(P[:, 1], R)
    ang = (np.repeat(P[:, 2], R) + np.tile(rel, A)).astype(f32)
    dx, dy = np.cos(ang).astype(f32), (-np.sin(ang)).astype(f32)
    stp = f32(stp)
    n = len(cx)

    def steps(s):
        with np.errstate(invalid="ignore"):
            return np.where(s >= stp, np.nan_to_num(s / stp, nan=0.0, posinf=1e6, neginf=0).astype(np.int64), 0)

    def probes(i, k, cnt):
        """Probes k .. k + cnt - 1 of beams i: (stop index or -1, point of the last probe)."""
        stop = np.full(len(i), -1, np.int64)
        for t in range(cnt):
            kk = k + t
            d = np.minimum(kk, S - 1).astype(f32) * stp
            fx, fy = cx[i] + dx[i] * d, cy[i] + dy[i] * d
            qx, qy = np.trunc(fx).astype(np.int64), np.trunc(fy).astype(np.int64)
            off = (qx < 0) | (qx >= W) | (qy < 0) | (qy >= W)
            hit = np.where(kk >= S, True, off | ((kk > 0) & ~on_road_px(qx, qy, rw)))
            stop = np.where((stop < 0) & hit, np.minimum(kk, S), stop)
        return stop, fx, fy

    px, py = cx.astype(np.int32), cy.astype(np.int32)
    onscr = (px >= 0) & (px < W) & (py >= 0) & (py < W)
    allb = np.arange(n)
    k = np.where(onscr, 1 + steps(safe1(cx, cy, dx, dy, rw)), 0)
    stop, lfx, lfy = probes(allb, k, NPR)
    k = k + NPR
    it = np.zeros(n, np.int32)
    act = stop < 0
    while act.any():
        i = np.nonzero(act)[0]
        it[i] += 1
        if pre:
            k[i] += steps(safe2(lfx[i], lfy[i], dx[i], dy[i], rw))
        st, fx, fy = probes(i, k[i], 2)
        k[i] += 2
        if not pre:
            k[i] += steps(safe2(fx, fy, dx[i], dy[i], rw))
        lfx[i], lfy[i] = fx, fy
        fin = (st >= 0) | (k[i] >= S)
        stop[i[fin]] = np.where(st[fin] >= 0, st[fin], S)
        act[i[fin]] = False
    return it, stop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--steps", type=int, default=300)
    a = ap.parse_args()
    N, R = 8, 64
    P = poses(a.envs, a.steps, n=N, rays=R)
    rel = np.array([np.float32(np.float32(-180.0) + np.float32(i) * np.float32(360.0 / (R - 1))) for i in range(R)],
                   np.float32) * np.float32(np.pi / 180.0)
    _, base_stop = march(P, rel, safe_v0, safe_v0)
    print(f"{len(P)} agent poses x {R} beams; an 'env' below = {N} consecutive poses")
    for name, s1, s2, pre in [("road_safe (current)", safe_v0, safe_v0, False),
                              ("exact-axes margins", safe_v1, safe_v1, False),
                              ("entry bound, placement (a)", safe_entry, safe_entry, False),
                              ("entry bound, placement (b)", safe_v0, safe_entry, True)]:
        it, stop = march(P, rel, s1, s2, pre)
        assert (stop == base_stop).all(), f"{name}: stop index differs from the current bound"
        ne = len(P) // N
        q = (it > 0)[:ne * N * R].reshape(ne, N * R).sum(1)
        itb = it[:ne * N * R].reshape(ne, N * R)
        print(f"{name:28s} queued beams per env mean {q.mean():.1f} p90 {np.percentile(q, 90):.0f} max {q.max()}; "
              f"beam-iterations per env {itb.sum(1).mean():.1f}; longest beam's iterations per env {itb.max(1).mean():.2f}")


if __name__ == "__main__":
    main()
