"""TEST INFRASTRUCTURE: a numpy float32 restatement of the renderer semantics written out in renderih_amd/render.py (pytorch3d
0.7.2 hard rasteriser, HardPhongShader / AmbientLights, hard_rgb_blend) -- the oracle of tests/test_render.py and
tests/test_gpu_render.py.  Not imported by the product.

rasterize() also reports, per pixel, how far the decision is from a rounding flip: `margin` = the smallest |min_i w_i| over
every face whose bounding box holds the pixel (a face within `margin` of an edge may be covered or not depending on the last
bit of an edge function), and `zgap` = the depth gap between the nearest and the second-nearest covering face."""
import numpy as np

f32 = np.float32


def orthographic_params(scale, trans2d):
    scale, trans2d = np.asarray(scale, f32).reshape(-1), np.asarray(trans2d, f32).reshape(-1, 2)
    B = scale.shape[0]
    p = np.zeros((B, 16), f32)
    p[:, 0], p[:, 4], p[:, 8], p[:, 11] = -1, -1, 1, 10
    p[:, 12] = p[:, 13] = 2 * scale
    p[:, 14:16] = -trans2d
    return p


def perspective_params(K, S):
    K = np.asarray(K, f32)
    B = K.shape[0]
    p = np.zeros((B, 16), f32)
    p[:, 0] = p[:, 4] = p[:, 8] = 1
    p[:, 12] = -K[:, 0, 0] * f32(2) / f32(S)
    p[:, 13] = -K[:, 1, 1] * f32(2) / f32(S)
    p[:, 14] = -K[:, 0, 2] * f32(2) / f32(S) + f32(1)
    p[:, 15] = -K[:, 1, 2] * f32(2) / f32(S) + f32(1)
    return p


def screen(verts, cam, persp):
    """verts [V, 3], cam [16] -> [V, 3] = NDC x, NDC y, view z."""
    X = np.asarray(verts, f32)
    R, T = cam[:9].reshape(3, 3), cam[9:12]
    xv = X[:, 0] * R[0, 0] + X[:, 1] * R[1, 0] + X[:, 2] * R[2, 0] + T[0]
    yv = X[:, 0] * R[0, 1] + X[:, 1] * R[1, 1] + X[:, 2] * R[2, 1] + T[1]
    zv = X[:, 0] * R[0, 2] + X[:, 1] * R[1, 2] + X[:, 2] * R[2, 2] + T[2]
    if persp:
        return np.stack([cam[12] * xv / zv + cam[14], cam[13] * yv / zv + cam[15], zv], -1).astype(f32)
    return np.stack([cam[12] * xv + cam[14], cam[13] * yv + cam[15], zv], -1).astype(f32)


def pixel_centres(S):
    return (f32(1) - (2 * np.arange(S) + 1).astype(f32) / f32(S)).astype(f32)


def rasterize(verts, faces, cams, persp, S):
    """verts [B, V, 3], faces [F, 3], cams [B, 16] -> dict of pix_to_face [B, S, S] (b F + f), zbuf, bary [B, S, S, 3],
    margin, zgap."""
    verts, faces, cams = np.asarray(verts, f32), np.asarray(faces, np.int64), np.asarray(cams, f32)
    B, F = verts.shape[0], faces.shape[0]
    ax = pixel_centres(S)
    out = {'pix_to_face': np.full((B, S, S), -1, np.int64), 'zbuf': np.full((B, S, S), -1, f32),
           'bary': np.full((B, S, S, 3), -1, f32), 'margin': np.full((B, S, S), np.inf, f32),
           'zgap': np.full((B, S, S), np.inf, f32)}
    half = f32(1) / f32(S)
    for b in range(B):
        s = screen(verts[b], cams[b], persp)[faces]                  # [F, 3 corners, 3]
        x, y, z = s[..., 0], s[..., 1], s[..., 2]
        area = (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0]) - (y[:, 2] - y[:, 0]) * (x[:, 1] - x[:, 0])
        skip = np.abs(area) < f32(1e-8)
        if persp:
            skip |= (z <= 0).any(1)
        ia = f32(1) / (area + f32(1e-8))
        best = np.full((S, S), np.inf, f32)
        second = np.full((S, S), np.inf, f32)
        bf = np.full((S, S), -1, np.int64)
        bw = np.full((S, S, 3), -1, f32)
        margin = out['margin'][b]
        for f in np.nonzero(~skip)[0]:
            # columns / rows whose centre lies in the box (half a pixel of margin, as the kernel's tile cull)
            cols = np.nonzero((ax >= x[f].min() - half) & (ax <= x[f].max() + half))[0]
            rows = np.nonzero((ax >= y[f].min() - half) & (ax <= y[f].max() + half))[0]
            if cols.size == 0 or rows.size == 0:
                continue
            px, py = ax[cols][None, :], ax[rows][:, None]
            x0, y0, x1, y1, x2, y2 = x[f, 0], y[f, 0], x[f, 1], y[f, 1], x[f, 2], y[f, 2]
            w0 = ((px - x1) * (y2 - y1) - (py - y1) * (x2 - x1)) * ia[f]
            w1 = ((px - x2) * (y0 - y2) - (py - y2) * (x0 - x2)) * ia[f]
            w2 = ((px - x0) * (y1 - y0) - (py - y0) * (x1 - x0)) * ia[f]
            m = np.minimum(np.minimum(w0, w1), w2)
            sub = np.ix_(rows, cols)
            margin[sub] = np.minimum(margin[sub], np.abs(m))
            cov = m >= 0
            if persp:
                z0, z1, z2 = z[f]
                t0, t1, t2 = w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2
                d = np.maximum(t0 + t1 + t2, f32(1e-8))
                w0, w1, w2 = t0 / d, t1 / d, t2 / d
            zz = w0 * z[f, 0] + w1 * z[f, 1] + w2 * z[f, 2]
            cov &= zz >= 0
            bsub, ssub = best[sub], second[sub]
            win = cov & (zz < bsub)                  # faces in ascending order: a tie keeps the lower index
            ssub = np.where(win, bsub, np.where(cov, np.minimum(ssub, zz), ssub))
            bsub = np.where(win, zz, bsub)
            best[sub], second[sub] = bsub, ssub
            bfs, bws = bf[sub], bw[sub]
            bfs[win] = f
            bws[win] = np.stack([w0, w1, w2], -1)[win]
            bf[sub], bw[sub] = bfs, bws
        hit = bf >= 0
        out['pix_to_face'][b] = np.where(hit, b * F + bf, -1)
        out['zbuf'][b] = np.where(hit, best, f32(-1))
        out['bary'][b] = bw
        with np.errstate(invalid='ignore'):
            out['zgap'][b] = np.where(hit, second - best, np.inf)
    return out


def vertex_normals(verts, faces):
    """Meshes.verts_normals: per vertex the sum of the corner cross products (p1 - p0) x (p2 - p0) of its faces, in ascending
    (face, corner) order, normalised with eps 1e-6.  verts [B, V, 3] -> [B, V, 3]."""
    verts, faces = np.asarray(verts, f32), np.asarray(faces, np.int64)
    out = np.zeros_like(verts)
    for b in range(verts.shape[0]):
        v = verts[b]
        p0 = v[faces]
        p1 = v[faces[:, [1, 2, 0]]]
        p2 = v[faces[:, [2, 0, 1]]]
        cr = np.cross(p1 - p0, p2 - p0).astype(f32)          # [F, 3 corners, 3]
        n = np.zeros_like(v)
        np.add.at(n, faces.reshape(-1), cr.reshape(-1, 3))   # entry 3 f + corner, applied in that order
        out[b] = _normalize(n)
    return out


def _normalize(v):
    return (v / np.maximum(np.sqrt((v * v).sum(-1, keepdims=True)), f32(1e-6))).astype(f32)


def shade(frags, verts, faces, colors, cams, ambient):
    """RGBA [B, S, S, 4] (hard_rgb_blend; RGB not divided by 255)."""
    verts, faces, cams = np.asarray(verts, f32), np.asarray(faces, np.int64), np.asarray(cams, f32)
    B, V = verts.shape[:2]
    F = faces.shape[0]
    colors = np.broadcast_to(np.asarray(colors, f32), (B, V, 3))
    p2f, w = frags['pix_to_face'], frags['bary']
    S = p2f.shape[1]
    rgba = np.zeros((B, S, S, 4), f32)
    rgba[..., :3] = 1
    normals = None if ambient else vertex_normals(verts, faces)
    for b in range(B):
        hit = p2f[b] >= 0
        f = p2f[b][hit] - b * F
        vi = faces[f]                                          # [P, 3]
        wb = w[b][hit][..., None]                              # [P, 3, 1]
        c = colors[b][vi]                                      # [P, 3 corners, 3]
        tex = c[:, 0] + wb[:, 1] * (c[:, 1] - c[:, 0]) + wb[:, 2] * (c[:, 2] - c[:, 0])
        if ambient:
            col = tex
        else:
            P = (wb * verts[b][vi]).sum(1)
            N = _normalize((wb * normals[b][vi]).sum(1))
            L = _normalize(np.array([0, 0, -1], f32) - P)
            R, T = cams[b, :9].reshape(3, 3), cams[b, 9:12]
            C = -(T[None, :] * R).sum(1)                       # -T R^T
            Vd = _normalize(C[None, :] - P)
            cosl = (N * L).sum(-1)
            diffuse = f32(0.3) * np.maximum(cosl, 0)
            r = -L + 2 * cosl[:, None] * N
            a = np.maximum((Vd * r).sum(-1), 0) * (cosl > 0)
            a = a.astype(f32)
            for _ in range(6):                                 # a^64 as six squarings
                a = a * a
            spec = f32(0.2) * a
            col = (f32(0.5) + diffuse)[:, None] * tex + spec[:, None]
        rgba[b][hit, :3] = col
        rgba[b][hit, 3] = 1
    return rgba
