"""The twin-scene construction of the first-hit oracle (no GPU; tests/test_gpu_features.py explains it).

A TWIN scene -- same primitives and BVH, every material replaced by LAMBERT with base colour 0 and
emission e_i -- makes the oracle's getColor return e_i of the first primitive hit and stop, or 0 on a miss.
"""
import ctypes as C

from oracle import pyoracle as po


def twin(osc, emission):
    """The scene with every material LAMBERT, base colour 0, no texture, emission[i]; no sky."""
    t = po.OracleScene()
    t.camera, t.nodes, t.node_count, t.prim_count = osc.camera, osc.nodes, osc.node_count, osc.prim_count
    prims = (po.Hittable * osc.prim_count).from_buffer_copy(bytes(osc.prims)[:osc.prim_count * C.sizeof(po.Hittable)])
    for i in range(osc.prim_count):
        m = prims[i].mat
        m.baseColor[:] = [0.0, 0.0, 0.0]
        m.emissive[:] = [float(v) for v in emission[i]]
        m.textureIndex, m.materialType = 0, 0
    t.prims = prims
    return t


def first_hits(osc, emission, W, H, tiling, camera=None):
    """The twin's one-sample reset render: emission of the first primitive each pixel's first ray hits."""
    ref = po.OracleRenderer(twin(osc, emission), W, H, tiling[1], tiling[2], band_rows=tiling[0])
    ref.render(osc.camera if camera is None else camera, 1, True)
    return ref.accum
