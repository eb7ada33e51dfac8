"""numpy fp32 restatement of the closest-hit / miss shader without a secondary ray (closest.cpp:57-127 else arm, miss.cpp:9-14) and of
the RGB8 pack (common.h:149-154), in the manner of tests/camera_ref.py.  TEST INFRASTRUCTURE ONLY.

Written from the reference's shader text and the conversion rule of include/vortex_hip.h (vxrt_shade_rays), independently of
oracle/rt_oracle.c and csrc/rt_shading.h: one fp32 operation per line, no einsum, no contraction (numpy float32 arithmetic rounds
every operation).  tests/test_shading_cpu.py holds it bit-equal to pyoracle.shade; a misreading that the kernel and rt_oracle.c
shared would show there.  shade() also returns the intermediate values the liveness checks count."""
import numpy as np

f32 = np.float32
LARGE = f32(1e30)
MAT_DT = np.dtype([("f", "<f4", 16), ("tex_id", "<i4"), ("illum", "<i4"), ("tw", "<u4"), ("th", "<u4"), ("off", "<u8")])


def f2u_x86(x):
    """uint32_t(float): the truncated value mod 2^32 for -2^63 <= x < 2^63, 0 for NaN and everything else"""
    x = np.asarray(x, np.float32)
    ok = (x >= f32(-2.0 ** 63)) & (x < f32(2.0 ** 63))
    t = np.trunc(np.where(ok, x, f32(0))).astype(np.int64)
    return (t & 0xFFFFFFFF).astype(np.uint32)


def f2i_x86(x):
    """int(float) as its 32 bits: the truncated value for -2^31 <= x < 2^31, INT_MIN for NaN and everything else"""
    x = np.asarray(x, np.float32)
    ok = (x >= f32(-2.0 ** 31)) & (x < f32(2.0 ** 31))
    t = np.trunc(np.where(ok, x, f32(0))).astype(np.int64)
    return np.where(ok, t & 0xFFFFFFFF, 0x80000000).astype(np.uint32)


def pack_rgb8(col):
    """(int(min(r, 1) * 255) << 16) + (int(min(g, 1) * 255) << 8) + int(min(b, 1) * 255) in 32-bit registers;
    std::min(c, 1.f) = (1.f < c) ? 1.f : c"""
    col = np.asarray(col, np.float32)
    with np.errstate(all="ignore"):
        c = np.where(f32(1.0) < col, f32(1.0), col)
        q = c * f32(255)
    i = f2i_x86(q).astype(np.uint64)
    return (((i[:, 0] << np.uint64(16)) + (i[:, 1] << np.uint64(8)) + i[:, 2]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _col(a, stride, byte_off, idx, dtype):
    """field at byte_off of record idx of a packed record array"""
    raw = np.frombuffer(np.ascontiguousarray(a, np.uint8).tobytes(), np.uint8)
    return raw[(idx.astype(np.int64) * stride + byte_off)[:, None] + np.arange(4)].copy().view(dtype)[:, 0]


def shade(scene, rays, hits, params):
    """colours (n, 3) f32, rgb8 (n,) u32, and a dict of intermediates (arrays over the rays that hit)"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = len(rays)
    amb, lcol, lpos, bg = (np.asarray(v, np.float32) for v in (params.ambient, params.light_color, params.light_pos, params.background))
    col = np.zeros((n, 3), np.float32)
    found = hits["dist"] != LARGE
    col[~found] = bg
    fi = np.nonzero(found)[0]
    info = {"found": fi}
    if len(fi) == 0:
        return col, pack_rgb8(col), info
    r, h = rays[fi], hits[fi]
    bi, ti = h["blasIdx"], h["triIdx"]
    bx, by, bz, dist_hit = h["bx"], h["by"], h["bz"], h["dist"]
    ex = [_col(scene["triEx"], 64, 4 * k, ti, np.float32) for k in range(15)]     # N0, N1, N2, uv0, uv1, uv2
    tex_id = _col(scene["triEx"], 64, 60, ti, np.uint32)
    m = [_col(scene["blas"], 160, 4 + 4 * k, bi, np.float32) for k in range(16)]   # invTransform, row-major
    refl = _col(scene["blas"], 160, 152, bi, np.float32)
    mat = np.frombuffer(np.ascontiguousarray(scene["mat"], np.uint8).tobytes(), MAT_DT)[tex_id]
    tex = np.frombuffer(np.ascontiguousarray(scene["tex"], np.uint8).tobytes(), np.uint8)
    with np.errstate(all="ignore"):
        # I = orig + dir * dist
        I = []
        for k in range(3):
            t = r[:, 3 + k] * dist_hit
            I.append(r[:, k] + t)
        # N = N1 * bx + N2 * by + N0 * bz
        N = []
        for k in range(3):
            a = ex[3 + k] * bx
            b = ex[6 + k] * by
            c = ex[k] * bz
            s = a + b
            N.append(s + c)
        # TransformVector(N, invTransform.transposed()): column k of the 3 x 3 block, w = 0
        T = []
        for k in range(3):
            a = m[k] * N[0]
            b = m[4 + k] * N[1]
            c = m[8 + k] * N[2]
            z = f32(0.0) * f32(0.0)
            s = a + b
            s = s + c
            T.append(s + z)
        # normalize: v * (1 / sqrt(dot(v, v)))
        xx = T[0] * T[0]
        yy = T[1] * T[1]
        zz = T[2] * T[2]
        d2 = xx + yy
        d2 = d2 + zz
        tlen = np.sqrt(d2)
        inv = f32(1.0) / tlen
        Nn = [T[k] * inv for k in range(3)]
        # uv = uv1 * bx + uv2 * by + uv0 * bz
        uv = []
        for k in range(2):
            a = ex[11 + k] * bx
            b = ex[13 + k] * by
            c = ex[9 + k] * bz
            s = a + b
            uv.append(s + c)
        # texColor: texSample + RGB8toRGB32F for a textured material, the material's diffuse colour otherwise
        textured = mat["tex_id"] >= 0
        tw = np.where(textured, mat["tw"], 1).astype(np.uint32)
        th = np.where(textured, mat["th"], 1).astype(np.uint32)
        uw = uv[0] * tw.astype(np.float32)
        vh = uv[1] * th.astype(np.float32)
        iu = f2u_x86(uw) % tw
        iv = f2u_x86(vh) % th
        texel_index = iu.astype(np.int64) + iv.astype(np.int64) * tw.astype(np.int64)
        byte = np.where(textured, mat["off"].astype(np.int64) + 4 * texel_index, 0)
        texel = tex[byte[:, None] + np.arange(4)].copy().view(np.uint32)[:, 0]
        scale = f32(1.0) / f32(256.0)
        tc = []
        for k, shift in enumerate((16, 8, 0)):
            ch = ((texel >> np.uint32(shift)) & np.uint32(255)).astype(np.int32).astype(np.float32) * scale
            tc.append(np.where(textured, ch, mat["f"][:, 3 + k]).astype(np.float32))
        # diffuseLighting
        L = [lpos[k] - I[k] for k in range(3)]
        xx = L[0] * L[0]
        yy = L[1] * L[1]
        zz = L[2] * L[2]
        d2 = xx + yy
        d2 = d2 + zz
        dist = np.sqrt(d2)
        il = f32(1.0) / dist
        Ln = [L[k] * il for k in range(3)]
        t = dist * f32(0.1)
        t = f32(1.0) + t
        att = f32(1.0) / t
        a = Nn[0] * Ln[0]
        b = Nn[1] * Ln[1]
        c = Nn[2] * Ln[2]
        s = a + b
        ndl_raw = s + c
        ndl = np.where(f32(0.0) < ndl_raw, ndl_raw, f32(0.0)).astype(np.float32)      # std::max(0.f, x) = (0.f < x) ? x : 0.f
        out = []
        for k in range(3):
            la = lcol[k] * att
            la = la * ndl
            s = amb[k] + la
            dif = tc[k] * s
            dif = dif * f32(1.0)             # throughput
            om = f32(1.0) - refl
            term = dif * om
            rad = f32(0.0) + term
            thr = f32(1.0) * refl
            back = bg[k] * thr
            out.append(rad + back)
        col[fi] = np.stack(out, 1)
    info.update(textured=textured, material=tex_id, tw=tw, th=th, u=uv[0], v=uv[1], uw=uw, vh=vh, ndl_raw=ndl_raw, tlen=tlen,
                light_dist=dist, texel_index=texel_index)
    return col, pack_rgb8(col), info
