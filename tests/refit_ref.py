"""numpy restatement of the refit (vxrt_accel_refit / vxrt_accel_set_transforms, csrc/rt_accel.hip) in fp32 without fused
operations: the quantiser the GPU builder and the refit share (csrc/bvh_quant.h: bb_pick_exp, bb_quant_axis and the exponent bump
loop), the MESA inverse (mat4_t::inverted), the corner transform of an instance box (TransformPosition) and a whole bottom-up refit
of a reference-format scene's tlas / bvh buffers.  Not a test module: the refit tests import it."""
import numpy as np

NODE = np.dtype([("o", "<f4", 3), ("e", "i1", 3), ("imask", "u1"), ("lf", "<u4"), ("ld", "<u4"), ("ch", "u1", (4, 7))])
assert NODE.itemsize == 52
BLAS_WORDS = 40
F = np.float32
TLAS_INTERNAL = 0xFFFFFFFF


class RefitError(ValueError):
    """A non-finite vertex, transform or box, a singular matrix or a box that cannot be quantised: the refit returns -1."""


def pick_exp(extent):
    """bb_pick_exp: smallest e with extent / 255 <= 2^e, clamped to [-126, 126] (-126 where the fp32 quotient underflows to 0); 0 for
    an extent that is not > 0 or above 3e38."""
    ext = np.asarray(extent, F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        q = ext / F(255.0)
        m, k = np.frexp(q)
        e = np.where(m == F(0.5), k - 1, k)
        e = np.where(q == 0, -126, np.clip(e, -126, 126))
        bad = ~(ext > 0) | (ext > F(3.0e38))
    return np.where(bad, 0, e).astype(np.int32)


def pow2(e):
    return np.ldexp(F(1), np.asarray(e, np.int32)).astype(F)


def quant_axis(origin, s, inv, cmin, cmax):
    """bb_quant_axis over arrays: (q_lo, q_hi, ok)."""
    origin, s, inv, cmin, cmax = (np.asarray(x, F) for x in (origin, s, inv, cmin, cmax))
    with np.errstate(invalid="ignore", over="ignore"):
        fl = np.floor((cmin - origin) * inv).astype(F)
        fh = np.ceil((cmax - origin) * inv).astype(F)
        fl = np.where(fl >= 0, fl, F(0))
        fh = np.where(fh >= fl, fh, fl)
        ok = ~(fh > 255) & ~(fl > 255)
        lo = np.where(ok, fl, F(0))
        hi = np.where(ok, fh, F(0))
        while True:                                      # conservative after the decode's own rounding
            m = ok & (lo > 0) & ((origin + lo * s) > cmin)
            if not m.any():
                break
            lo = np.where(m, lo - 1, lo).astype(F)
        while True:
            m = ok & (hi < 255) & ((origin + hi * s) < cmax)
            if not m.any():
                break
            hi = np.where(m, hi + 1, hi).astype(F)
        ok &= ~((origin + hi * s) < cmax)
    return lo.astype(np.int64), hi.astype(np.int64), ok


def quant_children(origin, e, cmin, cmax, present):
    """The exponent bump loop of one axis for m nodes: origin [m], e [m] (start), cmin / cmax [m, 4], present [m, 4] bool.
    Returns (e, ql [m, 4], qh [m, 4], ok [m])."""
    e = np.array(e, np.int32)
    m = len(e)
    ql = np.zeros((m, 4), np.int64)
    qh = np.zeros((m, 4), np.int64)
    done = np.zeros(m, bool)
    ok = np.ones(m, bool)
    todo = np.arange(m)
    while len(todo):
        s, inv = pow2(e[todo]), pow2(-e[todo])
        lo, hi, good = quant_axis(origin[todo, None], s[:, None], inv[:, None], cmin[todo], cmax[todo])
        good = good | ~present[todo]
        fit = good.all(1)
        # (the kernel stops at the first child that does not fit; the bytes of a node that fits are the same)
        ql[todo[fit]] = np.where(present[todo[fit]], lo[fit], 0)
        qh[todo[fit]] = np.where(present[todo[fit]], hi[fit], 0)
        done[todo[fit]] = True
        stuck = ~fit & (e[todo] >= 126)
        ok[todo[stuck]] = False
        done[todo[stuck]] = True
        e[todo[~fit & ~stuck]] += 1
        todo = todo[~done[todo]]
    return e, ql, qh, ok


def inverted(c):
    """mat4_t::inverted (geometry.h:1149-1192, MESA) for matrices [n, 16] in fp32, operation order kept.
    Returns (inverse [n, 16], det [n])."""
    c = [np.asarray(c, F).reshape(-1, 16)[:, k].copy() for k in range(16)]
    with np.errstate(all="ignore"):
        inv = [
            c[5] * c[10] * c[15] - c[5] * c[11] * c[14] - c[9] * c[6] * c[15] + c[9] * c[7] * c[14] + c[13] * c[6] * c[11] - c[13] * c[7] * c[10],
            -c[1] * c[10] * c[15] + c[1] * c[11] * c[14] + c[9] * c[2] * c[15] - c[9] * c[3] * c[14] - c[13] * c[2] * c[11] + c[13] * c[3] * c[10],
            c[1] * c[6] * c[15] - c[1] * c[7] * c[14] - c[5] * c[2] * c[15] + c[5] * c[3] * c[14] + c[13] * c[2] * c[7] - c[13] * c[3] * c[6],
            -c[1] * c[6] * c[11] + c[1] * c[7] * c[10] + c[5] * c[2] * c[11] - c[5] * c[3] * c[10] - c[9] * c[2] * c[7] + c[9] * c[3] * c[6],
            -c[4] * c[10] * c[15] + c[4] * c[11] * c[14] + c[8] * c[6] * c[15] - c[8] * c[7] * c[14] - c[12] * c[6] * c[11] + c[12] * c[7] * c[10],
            c[0] * c[10] * c[15] - c[0] * c[11] * c[14] - c[8] * c[2] * c[15] + c[8] * c[3] * c[14] + c[12] * c[2] * c[11] - c[12] * c[3] * c[10],
            -c[0] * c[6] * c[15] + c[0] * c[7] * c[14] + c[4] * c[2] * c[15] - c[4] * c[3] * c[14] - c[12] * c[2] * c[7] + c[12] * c[3] * c[6],
            c[0] * c[6] * c[11] - c[0] * c[7] * c[10] - c[4] * c[2] * c[11] + c[4] * c[3] * c[10] + c[8] * c[2] * c[7] - c[8] * c[3] * c[6],
            c[4] * c[9] * c[15] - c[4] * c[11] * c[13] - c[8] * c[5] * c[15] + c[8] * c[7] * c[13] + c[12] * c[5] * c[11] - c[12] * c[7] * c[9],
            -c[0] * c[9] * c[15] + c[0] * c[11] * c[13] + c[8] * c[1] * c[15] - c[8] * c[3] * c[13] - c[12] * c[1] * c[11] + c[12] * c[3] * c[9],
            c[0] * c[5] * c[15] - c[0] * c[7] * c[13] - c[4] * c[1] * c[15] + c[4] * c[3] * c[13] + c[12] * c[1] * c[7] - c[12] * c[3] * c[5],
            -c[0] * c[5] * c[11] + c[0] * c[7] * c[9] + c[4] * c[1] * c[11] - c[4] * c[3] * c[9] - c[8] * c[1] * c[7] + c[8] * c[3] * c[5],
            -c[4] * c[9] * c[14] + c[4] * c[10] * c[13] + c[8] * c[5] * c[14] - c[8] * c[6] * c[13] - c[12] * c[5] * c[10] + c[12] * c[6] * c[9],
            c[0] * c[9] * c[14] - c[0] * c[10] * c[13] - c[8] * c[1] * c[14] + c[8] * c[2] * c[13] + c[12] * c[1] * c[10] - c[12] * c[2] * c[9],
            -c[0] * c[5] * c[14] + c[0] * c[6] * c[13] + c[4] * c[1] * c[14] - c[4] * c[2] * c[13] - c[12] * c[1] * c[6] + c[12] * c[2] * c[5],
            c[0] * c[5] * c[10] - c[0] * c[6] * c[9] - c[4] * c[1] * c[10] + c[4] * c[2] * c[9] + c[8] * c[1] * c[6] - c[8] * c[2] * c[5]]
        det = c[0] * inv[0] + c[1] * inv[4] + c[2] * inv[8] + c[3] * inv[12]
        invdet = F(1) / det
        out = np.stack([v * invdet for v in inv], 1).astype(F)
    return out, det


def set_transforms(blas, first, mats):
    """vxrt_accel_set_transforms on the host: the instance records (uint8 buffer, 160 B each) after writing `mats` ([n, 16] or
    [n, 4, 4], fp32) from record `first` on.  Raises RefitError where the call returns -1 (records then unchanged)."""
    m = np.asarray(mats, F).reshape(-1, 16)
    inv, det = inverted(m)
    if not np.isfinite(m).all() or (det == 0).any() or not np.isfinite(inv).all():
        raise RefitError("a non-finite or singular transform")
    out = np.array(blas, np.uint8).copy()
    rec = out.view(F).reshape(-1, BLAS_WORDS)
    rec[first:first + len(m), 1:17] = inv
    rec[first:first + len(m), 17:33] = m
    return out


def transform_box(m, lo, hi):
    """World box of object boxes lo / hi [n, 3] under matrices m [n, 16]: the 8 corners through TransformPosition (geometry.h:
    1280-1289), ((c0 x + c1 y) + c2 z) + c3, fp32, then min / max (bvh.cpp:295-304)."""
    m = np.asarray(m, F).reshape(-1, 16)
    wl = np.full((len(m), 3), np.inf, F)
    wh = np.full((len(m), 3), -np.inf, F)
    with np.errstate(all="ignore"):
        for c in range(8):
            x = np.where(c & 1, hi[:, 0], lo[:, 0]).astype(F)
            y = np.where(c & 2, hi[:, 1], lo[:, 1]).astype(F)
            z = np.where(c & 4, hi[:, 2], lo[:, 2]).astype(F)
            for a in range(3):
                r = m[:, 4 * a: 4 * a + 4]
                p = ((r[:, 0] * x + r[:, 1] * y) + r[:, 2] * z) + r[:, 3]
                wl[:, a] = np.minimum(wl[:, a], p)
                wh[:, a] = np.maximum(wh[:, a], p)
    return wl, wh


def decode_children(n):
    """Decoded child boxes of nodes n (NODE records): lo, hi [m, 4, 3] and present [m, 4]."""
    s = np.ldexp(F(1), n["e"].astype(np.int32)).astype(F)
    q = n["ch"][:, :, 1:].astype(F)
    lo = (n["o"][:, None, :] + q[:, :, :3] * s[:, None, :]).astype(F)
    hi = (n["o"][:, None, :] + q[:, :, 3:] * s[:, None, :]).astype(F)
    return lo, hi, n["ch"][:, :, 0] != 0


def _walk(nodes, roots, bases, tlas):
    """Breadth-first from every root: leaves [k] and internal levels [(node, child 0)] from the roots down.  Raises RefitError on an
    internal node without a present child (the plan refuses such a tree before anything is written)."""
    idx = np.asarray(roots, np.int64)
    base = np.asarray(bases, np.int64)
    leaves, levels = [], []
    while len(idx):
        n = nodes[idx]
        leaf = (n["ld"] != TLAS_INTERNAL) if tlas else (n["ld"] != 0)
        leaves.append(idx[leaf])
        ii, bb, nn = idx[~leaf], base[~leaf], n[~leaf]
        c0 = bb + nn["lf"].astype(np.int64)
        levels.append((ii, c0))
        present = nn["ch"][:, :, 0] != 0
        if not present.any(1).all():
            raise RefitError("an internal node without a child")
        kids = c0[:, None] + np.arange(4)[None, :]
        idx = kids[present]
        base = np.repeat(bb, present.sum(1))
    return np.concatenate(leaves) if leaves else np.zeros(0, np.int64), levels


def _tri_boxes(tri, first, count):
    """min / max over the vertices of triangles [first, first + count) per leaf; ok = every vertex finite."""
    first, count = np.asarray(first, np.int64), np.asarray(count, np.int64)
    t = np.repeat(first - np.concatenate([[0], np.cumsum(count)[:-1]]), count) + np.arange(int(count.sum()))
    v = tri[t]                                            # [k, 3, 3]
    ok = bool(np.isfinite(v).all())
    starts = np.concatenate([[0], np.cumsum(count)[:-1]])
    lo = np.minimum.reduceat(v.min(1), starts, axis=0).astype(F)
    hi = np.maximum.reduceat(v.max(1), starts, axis=0).astype(F)
    return lo, hi, ok


def _set_origin(nodes, idx, lo, hi):
    nodes["o"][idx] = lo
    nodes["e"][idx] = np.stack([pick_exp(hi[:, a] - lo[:, a]) for a in range(3)], 1).astype(np.int8)


def _refit_levels(nodes, levels, fbox):
    for ii, c0 in reversed(levels):
        if not len(ii):
            continue
        n = nodes[ii]
        present = n["ch"][:, :, 0] != 0
        kids = np.where(present, c0[:, None] + np.arange(4)[None, :], c0[:, None])
        cb = fbox[kids]                                   # [m, 4, 6]
        clo = np.where(present[:, :, None], cb[:, :, :3], np.inf).astype(F)
        chi = np.where(present[:, :, None], cb[:, :, 3:], -np.inf).astype(F)
        lo, hi = clo.min(1), chi.max(1)
        ch = nodes["ch"]
        e_out = np.zeros((len(ii), 3), np.int32)
        for a in range(3):
            e0 = pick_exp(hi[:, a] - lo[:, a])
            e, ql, qh, ok = quant_children(lo[:, a], e0, np.where(present, clo[:, :, a], 0).astype(F),
                                           np.where(present, chi[:, :, a], 0).astype(F), present)
            if not ok.all():
                raise RefitError("a box cannot be quantised")
            e_out[:, a] = e
            for k in range(4):
                p = present[:, k]
                ch[ii[p], k, 1 + a] = ql[p, k]
                ch[ii[p], k, 4 + a] = qh[p, k]
        nodes["o"][ii] = lo
        nodes["e"][ii] = e_out.astype(np.int8)
        fbox[ii, :3], fbox[ii, 3:] = lo, hi


def refit(bufs, geometry=True):
    """The refit of a reference-format scene: bufs holds uint8 arrays tlas, blas, bvh, tri (others ignored).  Returns new (tlas, bvh)
    uint8 arrays -- the bytes vxrt_accel_refit(VXRT_REFIT_GEOMETRY if geometry else VXRT_REFIT_INSTANCES) leaves in the scene's
    buffers.  Raises RefitError where the call returns -1."""
    tlas = np.array(bufs["tlas"], np.uint8).copy().view(NODE)
    bvh = np.array(bufs["bvh"], np.uint8).copy().view(NODE)
    tri = np.asarray(bufs["tri"], np.uint8).view(F).reshape(-1, 3, 3)
    rec = np.asarray(bufs["blas"], np.uint8).view(F).reshape(-1, BLAS_WORDS)
    offs = rec[:, 0].view(np.uint32).astype(np.int64)
    fb_bvh = np.zeros((len(bvh), 6), F)
    bases = np.unique(offs)
    leaves, levels = _walk(bvh, bases, bases, tlas=False)    # (the plan walks every tree, whatever the refit moves)
    tleaves, _ = _walk(tlas, [0], [0], tlas=True)
    if geometry:
        if len(leaves):
            lo, hi, ok = _tri_boxes(tri, bvh["lf"][leaves], bvh["ld"][leaves])
            if not ok:
                raise RefitError("a non-finite vertex")
            _set_origin(bvh, leaves, lo, hi)
            fb_bvh[leaves, :3], fb_bvh[leaves, 3:] = lo, hi
        _refit_levels(bvh, levels, fb_bvh)
    inst = tlas["ld"][tleaves].astype(np.int64)
    root = offs[inst]
    if geometry:
        olo, ohi = fb_bvh[root, :3], fb_bvh[root, 3:]
        fin = True
    else:
        rn = bvh[root]
        olo = np.zeros((len(root), 3), F)
        ohi = np.zeros((len(root), 3), F)
        fin = True
        lf = rn["ld"] != 0
        if lf.any():
            lo, hi, fin = _tri_boxes(tri, rn["lf"][lf], rn["ld"][lf])
            olo[lf], ohi[lf] = lo, hi
        if (~lf).any():
            dlo, dhi, pres = decode_children(rn[~lf])
            olo[~lf] = np.where(pres[:, :, None], dlo, np.inf).min(1)
            ohi[~lf] = np.where(pres[:, :, None], dhi, -np.inf).max(1)
    m = rec[inst, 17:33]
    wl, wh = transform_box(m, olo, ohi)
    if not (fin and np.isfinite(m[:, :12]).all() and np.isfinite(wl).all() and np.isfinite(wh).all()):
        raise RefitError("a non-finite transform or box")
    bw = np.zeros((len(rec), 6), F)
    bw[inst, :3], bw[inst, 3:] = wl, wh
    return refit_tlas_from_boxes(tlas, bw[:, :3], bw[:, 3:]), bvh.view(np.uint8).reshape(-1)


def refit_tlas_from_boxes(tlas, wl, wh):
    """The TLAS half of the refit: new bytes (uint8) of the TLAS `tlas` (uint8 or NODE records; topology kept) whose leaf of instance i
    holds the world box wl[i] / wh[i] ([n_instances, 3] each, fp32), every internal node quantised bottom-up.  Also what
    vxrt_tlas_build must emit for its own topology.  Raises RefitError on a non-finite box or one that cannot be quantised."""
    tlas = np.array(np.asarray(tlas).view(np.uint8).reshape(-1), np.uint8).copy().view(NODE)
    wl, wh = np.asarray(wl, F), np.asarray(wh, F)
    tleaves, tlevels = _walk(tlas, [0], [0], tlas=True)
    inst = tlas["ld"][tleaves].astype(np.int64)
    if not (np.isfinite(wl[inst]).all() and np.isfinite(wh[inst]).all()):
        raise RefitError("a non-finite box")
    _set_origin(tlas, tleaves, wl[inst], wh[inst])
    fb_tlas = np.zeros((len(tlas), 6), F)
    fb_tlas[tleaves, :3], fb_tlas[tleaves, 3:] = wl[inst], wh[inst]
    _refit_levels(tlas, tlevels, fb_tlas)
    return tlas.view(np.uint8).reshape(-1)


def instance_boxes(bufs):
    """World boxes [n_blas, 2, 3] of every instance from its BLAS root's decoded box (the INSTANCES rule) -- what the TLAS must hold."""
    bvh = np.asarray(bufs["bvh"], np.uint8).view(NODE)
    tri = np.asarray(bufs["tri"], np.uint8).view(F).reshape(-1, 3, 3)
    rec = np.asarray(bufs["blas"], np.uint8).view(F).reshape(-1, BLAS_WORDS)
    root = rec[:, 0].view(np.uint32).astype(np.int64)
    rn = bvh[root]
    olo = np.zeros((len(root), 3), F)
    ohi = np.zeros((len(root), 3), F)
    lf = rn["ld"] != 0
    if lf.any():
        lo, hi, _ = _tri_boxes(tri, rn["lf"][lf], rn["ld"][lf])
        olo[lf], ohi[lf] = lo, hi
    if (~lf).any():
        dlo, dhi, pres = decode_children(rn[~lf])
        olo[~lf] = np.where(pres[:, :, None], dlo, np.inf).min(1)
        ohi[~lf] = np.where(pres[:, :, None], dhi, -np.inf).max(1)
    return transform_box(rec[:, 17:33], olo, ohi)
