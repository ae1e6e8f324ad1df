"""Exactly periodic images for the Fast A-KAZE arm: every pixel away from the border sees the same float operations as the pixel one
period away, so the determinant plane repeats bit for bit and candidates of EQUAL response meet inside each other's radius.  The
in-level rule of Find_Scale_Space_Extrema keeps the earlier point then (`p.response > kept.response`, oracle/akaze.c); the parallel
forms on the device have to preserve that.  No other image of the suite produces an equal response.

tie_events() replays the rule over the oracle's determinant planes (akaze_detect(dbg_level=...)) and counts what it meets."""
import numpy as np

H, W = 240, 320
THRESHOLDS = (1e-20, 0.0)


def lattice_images():
    """{"tile3": a random 3 x 3 tile repeated over the image, "diag13": T[(x + 5 y) mod 13] with 13 random levels}"""
    rng = np.random.default_rng(20261)
    tile = rng.random((3, 3)).astype(np.float32)
    tile3 = np.tile(tile, (H // 3 + 1, W // 3 + 1))[:H, :W]
    T = rng.random(13).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    diag13 = T[(xx + 5 * yy) % 13]
    return {"tile3": np.ascontiguousarray(tile3, np.float32), "diag13": np.ascontiguousarray(diag13, np.float32)}


def tie_events(oracle, img, threshold):
    """-> dict(candidates, hits, ties, replacements, subnormal): candidates of all levels in the oracle's raster order; `hits` found a
    kept point within their size, `ties` of them with an equal response (the kept point stays), `replacements` with a larger one;
    `subnormal`: determinant values above the threshold that are subnormal floats"""
    f32 = np.float32
    thr = f32(threshold)
    nl = int(oracle.akaze_detect(img, threshold, dbg_level=0)["info"][0])
    tot = dict(candidates=0, hits=0, ties=0, replacements=0, subnormal=0)
    tiny = np.finfo(np.float32).tiny
    for lvl in range(nl):
        r = oracle.akaze_detect(img, threshold, dbg_level=lvl)
        d = r["ldet"]; info = r["info"]
        lh, lw = d.shape
        border = int(info[4]); psize = f32(info[6]) * f32(1.5); ratio = f32(2 ** (lvl // 4))
        s2 = psize * psize
        c = d[1:-1, 1:-1]
        mx = (c > thr)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if dy == 1 and dx == 1:
                    continue
                mx &= c > d[dy:dy + lh - 2, dx:dx + lw - 2]
        full = np.zeros((lh, lw), bool); full[1:-1, 1:-1] = mx
        inside = np.zeros((lh, lw), bool); inside[border:lh - border, border:lw - border] = True
        ys, xs = np.nonzero(full & inside)
        tot["subnormal"] += int(((d > thr) & (d < tiny)).sum())
        kx = np.zeros(len(ys), f32); ky = np.zeros(len(ys), f32); kr = np.zeros(len(ys), f32); n = 0
        for y, x in zip(ys.tolist(), xs.tolist()):
            px, py, resp = f32(x) * ratio, f32(y) * ratio, d[y, x]
            tot["candidates"] += 1
            ddx = px - kx[:n]; ddy = py - ky[:n]
            hit = np.flatnonzero(ddx * ddx + ddy * ddy <= s2)
            if len(hit):
                q = int(hit[0]); tot["hits"] += 1
                if resp == kr[q]:
                    tot["ties"] += 1
                elif resp > kr[q]:
                    tot["replacements"] += 1
                    kx[q], ky[q], kr[q] = px, py, resp
                continue
            kx[n], ky[n], kr[n] = px, py, resp; n += 1
    return tot
