"""A NumPy triangle rasteriser written from the rules of the object-coordinate renderer (csrc/raster.hpp states them): the
reference the renderer's tests compare isr_render_coords_host against.  A loop over faces, each face's pixel box vectorised,
edge functions in int64.  Besides the image it keeps, per pixel, the two smallest f64 depths among the covering fragments, so
a test can tell the pixels whose winner hangs on the last bit of a depth (depth-ambiguous pixels)."""
import numpy as np

SUB = 256
NEAR, FAR = 10.0, 10000.0


def project(verts, K, R, t):
    """f32 vertices -> (snapped x, snapped y (float, integral), camera z) in f64, the operation order of the rules."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    K, R, t = np.asarray(K, np.float64), np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3)
    cam = [((R[i, 0] * v[:, 0] + R[i, 1] * v[:, 1]) + R[i, 2] * v[:, 2]) + t[i] for i in range(3)]
    x, y, z = cam
    with np.errstate(all="ignore"):
        u = (K[0, 0] * x + K[0, 1] * y) / z + K[0, 2]
        w = (K[1, 0] * x + K[1, 1] * y) / z + K[1, 2]
        return np.rint(u * SUB), np.rint(w * SUB), z


def render(verts, faces, K, R, t, h, w, offset, scale, near=NEAR, far=FAR, state=None):
    """-> dict(color (h,w,4) f32, depth (h,w) f32, face (h,w) i64 (-1 empty, -2 kept from `state`), z1, z2 (h,w) f64 the two
    smallest fragment depths, color2 (h,w,3) f32 the colour of the second fragment, drawn, dropped, covered).
    state = (color, depth) of an earlier draw: this draw goes on top (clear = 0)."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64)
    sx, sy, z = project(verts, K, R, t)
    with np.errstate(all="ignore"):
        ok_v = (z >= near) & (np.abs(sx) < 2.0 ** 28) & (np.abs(sy) < 2.0 ** 28)
    attr = ((verts - np.asarray(offset, np.float32)) / np.float32(scale)).astype(np.float32).astype(np.float64)
    if state is None:
        color = np.zeros((h, w, 4), np.float32)
        depth = np.zeros((h, w), np.float32)
    else:
        color, depth = state[0].copy(), state[1].copy()
    old = (color[..., 3] == 1) & (depth > 0)
    best32 = np.where(old, depth, np.float32(np.inf)).astype(np.float32)
    face = np.where(old, -2, -1).astype(np.int64)
    z1 = np.where(old, depth.astype(np.float64), np.inf)
    z2 = np.full((h, w), np.inf)
    color2 = np.zeros((h, w, 3), np.float32)
    drawn = dropped = 0
    for f, (i0, i1, i2) in enumerate(faces):
        idx = [int(i0), int(i1), int(i2)]
        if min(idx) < 0 or max(idx) >= len(verts) or not ok_v[idx].all():
            dropped += 1
            continue
        drawn += 1
        X = [int(sx[i]) for i in idx]
        Y = [int(sy[i]) for i in idx]
        area2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
        if area2 == 0:
            continue
        if area2 < 0:
            idx[1], idx[2], X[1], X[2], Y[1], Y[2] = idx[2], idx[1], X[2], X[1], Y[2], Y[1]
            area2 = -area2
        c0, c1 = max(-(-min(X) // SUB), 0), min(max(X) // SUB, w - 1)
        r0, r1 = max(-(-min(Y) // SUB), 0), min(max(Y) // SUB, h - 1)
        if c0 > c1 or r0 > r1:
            continue
        py, px = np.meshgrid(np.arange(r0, r1 + 1, dtype=np.int64) * SUB, np.arange(c0, c1 + 1, dtype=np.int64) * SUB,
                             indexing="ij")
        lam, inside = [], True
        for a, b in ((1, 2), (2, 0), (0, 1)):               # the edge opposite vertex 0, 1, 2
            dx, dy = X[b] - X[a], Y[b] - Y[a]
            e = dx * (py - Y[a]) - dy * (px - X[a])
            top_left = dy < 0 or (dy == 0 and dx > 0)
            inside = inside & ((e >= 0) if top_left else (e > 0))
            lam.append(e)
        if not inside.any():
            continue
        zs = [z[i] for i in idx]
        rr, cc = np.nonzero(inside)
        wgt = [lam[k][rr, cc].astype(np.float64) / zs[k] for k in range(3)]
        S = (wgt[0] + wgt[1]) + wgt[2]
        zp = float(area2) / S
        keep = (zp >= near) & (zp <= far)
        rr, cc, zp, S = rr[keep] + r0, cc[keep] + c0, zp[keep], S[keep]
        wgt = [x[keep] for x in wgt]
        col = np.stack([(wgt[0] * attr[idx[0], k] + wgt[1] * attr[idx[1], k] + wgt[2] * attr[idx[2], k]) / S
                        for k in range(3)], axis=-1).astype(np.float32)
        z32 = zp.astype(np.float32)
        win = z32 < best32[rr, cc]                         # faces come in index order: only a strictly smaller depth wins
        # the two smallest f64 depths per pixel (and the colour of the one that is not the winner)
        lose = ~win
        sec = lose & (zp < z2[rr, cc])
        z2[rr[sec], cc[sec]] = zp[sec]
        color2[rr[sec], cc[sec]] = col[sec]
        wr, wc = rr[win], cc[win]
        demoted = z1[wr, wc] < z2[wr, wc]
        z2[wr[demoted], wc[demoted]] = z1[wr, wc][demoted]
        color2[wr[demoted], wc[demoted]] = color[wr, wc, :3][demoted]
        z1[wr, wc] = zp[win]
        best32[wr, wc] = z32[win]
        face[wr, wc] = f
        color[wr, wc, :3] = col[win]
        color[wr, wc, 3] = 1.0
        depth[wr, wc] = z32[win]
    return dict(color=color, depth=depth, face=face, z1=z1, z2=z2, color2=color2, drawn=drawn, dropped=dropped,
                covered=int((color[..., 3] == 1).sum()))


def ambiguous(ref):
    """Pixels whose two smallest fragment depths are within one f32 ulp of each other."""
    z1, z2 = ref["z1"], ref["z2"]
    with np.errstate(invalid="ignore"):
        ulp = np.spacing(np.where(np.isfinite(z1), z1, 1.0).astype(np.float32)).astype(np.float64)
        return np.isfinite(z1) & np.isfinite(z2) & (np.abs(z2 - z1) <= ulp)


def split_state(state, h, w):
    """The C frame-buffer block (5*h*w+4 words) -> (color (h,w,4) f32, depth (h,w) f32, counters (4,) i32)."""
    n = h * w
    return state[:4 * n].reshape(h, w, 4), state[4 * n:5 * n].reshape(h, w), state[5 * n:].view(np.int32)
