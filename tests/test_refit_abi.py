"""The C ABI of moving primitives without a rebuild (pt_set_primitive_boxes and its kin, include/pt_hip.h; the host
layer's functions, include/pt_host.h): the symbols are declared, exported and bound, the structs the calls take have the
sizes the kernels' packing assumes, and what can be refused without a device is refused."""
import ctypes as C
import re

import pathtracercuda_amd as pa
from pathtracercuda_amd import _native as N

SYMBOLS = ("pt_set_primitive_boxes", "pt_holds_primitive_boxes", "pt_move_primitives", "pt_read_bvh", "pt_read_primitive",
           "pt_read_refit_timing")
HOST_SYMBOLS = ("pth_renderer_move_objects", "pth_renderer_rebuild_scene", "pth_renderer_object_transforms",
                "pth_renderer_refit_timing", "pth_renderer_bvh", "pth_refit_boxes")


def test_symbols_are_declared_exported_and_bound(root):
    text = (root / "include" / "pt_hip.h").read_text()
    lib = N.hip()
    for name in SYMBOLS:
        assert re.search(rf"PT_API int {name}\(", text), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N._HIP_SYMBOLS and getattr(lib, name).argtypes == N._HIP_SYMBOLS[name][1]
    P = C.POINTER
    assert N._HIP_SYMBOLS["pt_move_primitives"][1] == [C.c_void_p, C.c_uint32, P(C.c_uint32), P(N.PtHittable), P(C.c_float),
                                                       P(C.c_float), P(C.c_uint32)]
    assert N._HIP_SYMBOLS["pt_read_bvh"][1] == [C.c_void_p, P(N.PtBvhNode), P(C.c_float)]
    host_text = (root / "include" / "pt_host.h").read_text()
    for name in HOST_SYMBOLS:
        assert re.search(rf"{name}\(", host_text) and hasattr(N.host(), name) and name in N._HOST_SYMBOLS
    assert "refit_boxes" in pa.__all__
    for name in ("move_objects", "object_transforms", "rebuild_scene", "refit_timing", "bvh"):
        assert callable(getattr(pa.Pathtracer, name))
    assert "10. The refit" in text                       # the rule is written where rules 1-9 are


def test_struct_sizes():
    # a node is two float4 on the device and a primitive's record four plus three: pt_read_bvh and pt_read_primitive
    # convert between these layouts, and a move packs 13 float4 (208 bytes) per primitive
    assert C.sizeof(N.PtBvhNode) == 32 and C.sizeof(N.PtHittable) == 96
    assert N.PtBvhNode.offset.offset == 24 and N.PtBvhNode.primitive_count_axis.offset == 28
    assert N.PtHittable.type.offset == 88


def test_refusals_that_need_no_device():
    lib = N.hip()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    buf, idx = (C.c_float * 32)(), (C.c_uint32 * 2)(0, 1)
    prims, nodes = (N.PtHittable * 2)(), (N.PtBvhNode * 2)()
    assert lib.pt_holds_primitive_boxes(None) == 0            # a question, never an error
    assert lib.pt_set_primitive_boxes(None, C.cast(buf, fp)) == N.PT_ERR_ARG
    assert lib.pt_move_primitives(None, 2, C.cast(idx, up), prims, C.cast(buf, fp), None, None) == N.PT_ERR_ARG
    assert lib.pt_read_bvh(None, nodes, None) == N.PT_ERR_ARG
    assert lib.pt_read_primitive(None, 0, C.cast(buf, fp)) == N.PT_ERR_ARG
    assert lib.pt_read_refit_timing(None, C.cast(buf, fp)) == N.PT_ERR_ARG
    assert not any(buf) and bytes(nodes) == bytes(32 * 2)
