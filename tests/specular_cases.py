"""The scenes and configurations of tests/test_specular_cpu.py and tests/test_gpu_specular.py.  TEST INFRASTRUCTURE ONLY.

All of it is emissive_cases.hall -- two mirrors, the ceiling light, the leaning lamp -- with the mirrors' reflectivities set:
  hall            the mirrors at 0.7 / 0.5, as the area-light tests have them
  mirrors = 1     the mirrors at exactly 1.0: every pick there is a mirror pick, the scene of identity C
  hidden mirror   the mirrors at 0 and one instance more, a 1 x 1 quad of reflectivity 0.5 at y = -1 under the middle of the floor, which
                  no path can reach: the scene of identity A.  An accel that holds it has a positive largest reflectivity, so a frame
                  that asked "is anything reflective" and took the old kernels would not make the identity vacuous."""
import types

import numpy as np

import emissive_cases as ec
import scenes

SCALE = ec.SCALE
FORMS = (None, "nee0", "nee1", "mis")
W, H = 16, 12
ODD_W, ODD_H, ODD_ROWS = 13, 7, (2, 6)
CONFIG = (4, 3, 7)                      # (spp, bounces, seed) of the frames against the restatement
DEEP = (1, 16, 5)                       # one sample, the most bounces
# counts of 1, between, the cap and above the cap (the mosaic identity and the restated counts frame)
COUNTS = {"values": (1, 3, 4, 9, 0xFFFFFFFF), "cap": 4, "bounces": 3, "shadow": 1, "seed": 7}
# paths per batch of the child process: spp = 5 of a 16 x 12 window in whole samples of 2, 2, 1 for the uniform tail (2 x 192 <= 400 <
# 3 x 192), and for the counts tail a capacity that is no multiple of any count, so that batch boundaries fall inside pixels
CHILD_BATCH = 400
CHILD_SPP = 5
HIDDEN = 6                              # the hidden mirror's instance record
EDGE_RHO = (1.0, 0.0, -0.3, float("nan"), float("inf"))


def _set_mirrors(b, front, back):
    rec = b["blas"].view(np.float32).reshape(-1, 40)
    rec[1, 38] = front
    rec[2, 38] = back


def hall(vrt, mirrors=(0.7, 0.5)):
    """(scene buffers, emitter pairs)"""
    b, ranges = ec.hall(vrt)
    _set_mirrors(b, *mirrors)
    return b, vrt.rtapi.emitter_pairs(b, ranges)


def hidden_mirror_hall(vrt):
    """(scene buffers, emitter pairs): emissive_cases.hall with one mesh more, handed to the same builder call"""
    quad = np.array(scenes._quad((274.5, -1, -0.5), (275.5, -1, -0.5), (275.5, -1, 0.5), (274.5, -1, 0.5)), np.float32)

    def from_triangles(meshes, xf, ex, mats):
        return vrt.scene.from_triangles(list(meshes) + [quad], list(xf) + [np.eye(4, dtype=np.float32)], list(ex) + [ec.tri_ex(quad, np.zeros(2, np.uint32))],
                                        list(mats) + [ec.material()])

    proxy = types.SimpleNamespace(scene=types.SimpleNamespace(procedural=vrt.scene.procedural, from_triangles=from_triangles))
    b, ranges = ec.hall(proxy)
    _set_mirrors(b, 0.0, 0.0)
    rec = b["blas"].view(np.float32).reshape(-1, 40)
    assert len(rec) == HIDDEN + 1
    rec[HIDDEN, 38] = 0.5
    return b, vrt.rtapi.emitter_pairs(b, ranges)


def counts_of(w=W, h=H, salt=0):
    import adaptive_cases as ac
    return ac.hashed(w, h, COUNTS["values"], salt)


def pick_vertices(n=4096, seed=5):
    """(vertices (n, 10), seeds (n,) u32) of the pick alone: random points, unit normals and directions, reflectivities over [0, 1.2) with
    the edge values of EDGE_RHO and exact ones mixed in, hash outputs with 0 among them"""
    rng = np.random.default_rng(seed)
    v = np.zeros((n, 10), np.float32)
    v[:, 0:3] = rng.uniform(-300, 300, (n, 3))
    for c in (3, 6):
        d = rng.normal(size=(n, 3))
        v[:, c:c + 3] = d / np.linalg.norm(d, axis=1)[:, None]
    v[:, 9] = rng.uniform(0.0, 1.2, n)
    v[::7, 9] = np.resize(np.array(EDGE_RHO + (-np.inf, 1e-30, 0.99999994), np.float32), len(v[::7]))
    seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    seeds[:4] = (0, 1, 0xFFFFFFFF, 0x80000000)
    v[0, 9], v[1, 9] = 0.5, 1.0
    return v, seeds
