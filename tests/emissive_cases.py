"""The scene and the configurations of tests/test_emissive_cpu.py and tests/test_gpu_emissive.py.  TEST INFRASTRUCTURE ONLY.

scenes.mirror_hall's four instances plus two more:
  4  the ceiling: a dark panel over the whole hall (material 0 of its mesh) with a light in it, a quad of 200 x 200 units above the blob
     (material 1, emissive) -- a mesh with emissive and plain triangles, so that listing the emitters has something to leave out;
  5  a unit quad of a second emissive material on an instance whose transform rotates it about z and x and scales it by (60, 25, 40):
     a lamp that leans against the side wall's corner, its world-space edges neither axis-aligned nor of the mesh's lengths.
The light of the ceiling can be cut into 2 k triangles (k x 1 strips of two), which gives the emitter tables of the scan's edges."""
import numpy as np

import scenes

CEILING, LAMP = 4, 5
LE_CEILING = (6.0, 5.5, 4.0)
LE_LAMP = (2.0, 3.0, 8.0)
SCALE = 1.0
# (spp, bounces, shadow, seed, nee)
CONFIGS = ((2, 3, 1, 3, 1), (5, 2, 0, 0, 1), (2, 2, 0, 1, 0))
TABLE_SIZES = (1, 2, 64, 65, 256, 257, 1025, 4097)


def material(diffuse=(0.8, 0.8, 0.8), emissive=(0.0, 0.0, 0.0)):
    """one material_info_t (88 B) without a texture"""
    m = np.zeros(22, np.float32)
    m[3:6] = diffuse
    m[9:12] = emissive
    m[14] = 1.0                                   # dissolve
    b = m.view(np.uint8).copy()
    b[64:68] = np.array([-1], np.int32).view(np.uint8)   # diffuse_tex_id
    return b


def tri_ex(tris, tex_ids):
    """tri_ex_t records of flat-shaded triangles: the geometric normal three times, uv1 = (1, 0), uv2 = (0, 1), texId"""
    t = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).astype(np.float64)
    n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(np.float32)
    e = np.zeros((len(t), 16), np.float32)
    e[:, 0:3] = e[:, 3:6] = e[:, 6:9] = n
    e[:, 11] = 1.0
    e[:, 14] = 1.0
    e.view(np.uint32)[:, 15] = np.asarray(tex_ids, np.uint32)
    return e.view(np.uint8).reshape(-1)


def light_strips(k):
    """the ceiling light (x 80..280, y 255, z -100..100, facing down) as k strips along x of two triangles each; k = 0.5: one triangle"""
    if k == 0.5:
        return np.array([[80, 255, -100, 280, 255, 100, 280, 255, -100]], np.float32)
    xs = (80.0 + 200.0 * (np.arange(int(k) + 1) / float(k)) ** 1.5).astype(np.float32)   # (strips of growing width: weights that differ)
    out = []
    for i in range(int(k)):
        out += scenes._quad((xs[i], 255, -100), (xs[i], 255, 100), (xs[i + 1], 255, 100), (xs[i + 1], 255, -100))
    return np.array(out, np.float32)


def lamp_transform():
    cz, sz, cx, sx = np.cos(0.5), np.sin(0.5), np.cos(-0.9), np.sin(-0.9)
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    m = np.eye(4)
    m[:3, :3] = rz @ rx @ np.diag([60.0, 25.0, 40.0])
    m[:3, 3] = (230.0, 150.0, 240.0)
    return m.astype(np.float32)


def hall(vrt, light_tris=2, emissive=True):
    """the scene buffers (dict of uint8 arrays) and the per-instance triangle ranges [(first, count)]; light_tris: triangles of the
    ceiling light (1, or an even number); emissive = False: the same geometry with both emissive colours zero"""
    blob = vrt.scene.procedural("blob", 2, 0, 3)
    bt = np.frombuffer(bytes(blob.buffers["tri"]), np.float32).reshape(-1, 3).copy()
    c = bt.mean(0)
    r = np.abs(bt - c).max()
    bt = ((bt - c) * np.float32(40.0 / r) + np.array([180.0, 90.0, 30.0], np.float32)).reshape(-1, 9).astype(np.float32)
    q = scenes._quad
    floor = np.array(q((-50, 0, -300), (600, 0, -300), (600, 0, 300), (-50, 0, 300)) +
                     q((-50, 0, 300), (600, 0, 300), (600, 260, 300), (-50, 260, 300)), np.float32)
    m1 = np.array(q((400, 10, -200), (400, 10, 200), (400, 230, 200), (400, 230, -200)), np.float32)
    m2 = np.array(q((-40, 10, -220), (-40, 240, -220), (-40, 240, 220), (-40, 10, 220)), np.float32)
    panel = np.array(q((-50, 260, -300), (-50, 260, 300), (600, 260, 300), (600, 260, -300)), np.float32)
    light = light_strips(0.5 if light_tris == 1 else light_tris // 2)
    assert len(light) == light_tris
    ceiling = np.concatenate([panel, light])
    lamp = np.array(q((-0.5, -0.5, 0), (0.5, -0.5, 0), (0.5, 0.5, 0), (-0.5, 0.5, 0)), np.float32)
    meshes = [floor, m1, m2, bt, ceiling, lamp]
    ids = [np.zeros(len(m), np.uint32) for m in meshes]
    ids[CEILING][len(panel):] = 1
    on = 1.0 if emissive else 0.0
    mats = [material()] * 4 + [np.concatenate([material((0.3, 0.3, 0.3)), material((0.8, 0.8, 0.8), tuple(on * v for v in LE_CEILING))]),
                               material((0.5, 0.5, 0.5), tuple(on * v for v in LE_LAMP))]
    xf = [np.eye(4, dtype=np.float32)] * 5 + [lamp_transform()]
    sc = vrt.scene.from_triangles(meshes, xf, [tri_ex(m, i) for m, i in zip(meshes, ids)], mats)
    b = {k: np.frombuffer(bytes(v), np.uint8).copy() for k, v in sc.buffers.items()}
    rec = b["blas"].view(np.float32).reshape(-1, 40)
    rec[1, 38] = 0.7                              # the mirrors of scenes.mirror_hall (a path frame reads the reflectivity in Lit)
    rec[2, 38] = 0.5
    first = np.concatenate([[0], np.cumsum([len(m) for m in meshes])[:-1]])
    return b, [(int(f), len(m)) for f, m in zip(first, meshes)]
