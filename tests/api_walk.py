"""Seeded walks over the render API: a generator of call sequences, a model of the state flags, and the
oracle's side of every successful call.  No GPU, and nothing of pathtracercuda_amd is imported here.

A device context and the host layer above it carry state from one call to the next:
  host    frames (the frame counter), m_adaptive, m_denoised
  device  "the counts describe the buffer" and "the moments can be continued" (two facts: include/pt_hip.h,
          adaptive sampling), the feature planes' validity, the denoised image's, the forced kernel variant
Model restates when each of them changes, from include/pt_hip.h, include/pathtracer_amd.hpp and DESIGN.md
5.6 / 5.7, and predicts for every call success or the PT_ERR_* code with a word of the message, and for the
image reads which arithmetic applies.  OracleWalk mirrors every successful call on the CPU oracle.
tests/test_api_walk.py checks the generator and the model; tests/test_gpu_api_walk.py walks the device.
"""
import ctypes as C
import json
import random
from collections import namedtuple

import numpy as np

import denoise_model as dm
from first_hit import first_hits
from oracle import pyoracle as po
from test_adaptive_rule import AdaptiveOracle

F = np.float32
PT_OK, PT_ERR_ARG, PT_ERR_STATE = 0, 2, 3

KINDS = ("render", "render_raw", "adaptive", "features", "denoise", "camera", "rng", "scene", "texture", "variant",
         "run_ahead", "groups", "knob")
SCENES = ("cornell_box", "test_shapes", "generated_scene")
START_SCENE = "test_shapes"            # it has textures: a texture call always finds an existing handle
SHIPPED_VARIANTS = (1, 4, 6, 20, 39, 40, 41, 46, 47, 48, 60, 61)      # pt_set_kernel_variant (pt_hip.h), without 91
ADAPTIVE_VARIANTS = (0, 4, 6, 40, 41, 46, 60, 61)                     # "honoured when it has an adaptive build"
# the scheduling knobs and their documented ranges (the setters in pt_kernels.hip state the bounds)
KNOBS = {"schedule": (0, 1), "strip_units": (0, 1, 2, 4, 16), "occupancy": (0, 1, 2, 4, 16),
         "cold_start": ((0, 1), (2, 1), (8, 0), (64, 1), (0, 0))}
TEXELS = ((0.5, 0.25, 0.75, 1.0), (0.9, 0.1, 0.2, 1.0), (0.05, 0.6, 0.3, 1.0))
DENOISE = dict(iterations=2, sigma_plane=0.03, normal_power_log2=3, demodulate=True, same_primitive=False)
DENOISE_SIGMA = 0.4
ADAPTIVE_FLOOR = 0.01

# Seeds and what each walks on.  seed % 8 picks the slice of the pair circuit and the named triples of a
# seed (build_walks), so eight consecutive seeds cover them all.
SEEDS = tuple(range(1984, 1992))
STEPS = 40                                       # of every walk at least; the repairs may add a few
Config = namedtuple("Config", "width height band_rows row_offset row_stride")
CONFIGS = {s: Config(60, 44, 1, 0, 1) for s in SEEDS}
CONFIGS[1990] = Config(60, 44, 8, 1, 2)          # a band partition: denoise is refused by name
CONFIGS[1991] = Config(7, 5, 1, 0, 1)            # less than one wave

Op = namedtuple("Op", "kind args")
Outcome = namedtuple("Outcome", "code word")
OK = Outcome(PT_OK, "")


def describe(op):
    return f"{op.kind}({', '.join(f'{k}={v!r}' for k, v in sorted(op.args.items()))})"


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------
class Model:
    """The flags, and for every call what it returns and what it changes.  A refused call changes nothing."""

    def __init__(self, whole_frame=True):
        self.whole_frame = whole_frame       # the context holds every row (pt_denoise needs that)
        self.frames = 0                      # host: m_accumulatedFrames
        self.made_adaptive = False           # host: m_adaptive
        self.denoised = False                # host: m_denoised -- the image calls return the denoised image
        self.counts_valid = False            # device: the per-pixel counts describe the buffer
        self.moments_valid = False           # device: the moments can be continued with reset = 0
        self.planes_valid = False            # device: feature planes of the current scene and textures
        self.planes_camera = None            # the camera they were made under (bytes)
        self.planes_read = False             # Python keeps the last planes it read (the automatic sigma's input)
        self.denoised_valid = False          # device: there is a denoised image
        self.variant = 0
        self.run_ahead = 0
        self.groups = 0

    @property
    def adaptive(self):
        """Pathtracer::adaptive(): this layer made an adaptive render and its counts still describe the buffer."""
        return self.made_adaptive and self.counts_valid

    def image(self):
        """Which arithmetic the image calls use: "denoised", "counts" (every pixel over its own n), "frames"."""
        return "denoised" if self.denoised else "counts" if self.adaptive else "frames"

    def color(self):
        """The image pt_denoise filters: never the denoised one."""
        return "counts" if self.counts_valid else "frames"

    def outcome(self, op):
        k, a = op.kind, op.args
        if k == "render" and self.adaptive and not a["ignore"]:
            return Outcome(PT_ERR_STATE, "adaptive")         # one frame counter cannot normalise such a buffer
        if k == "adaptive":
            if not a["reset"] and not (self.adaptive and self.moments_valid):
                return Outcome(PT_ERR_STATE, "reset")        # "PT_ERR_STATE when there are none"
            if self.variant not in ADAPTIVE_VARIANTS:
                return Outcome(PT_ERR_ARG, "adaptive build")
        if k == "denoise":
            auto = a["sigma"] is None
            if auto and not a["host"] and not self.planes_read:
                return Outcome(PT_ERR_STATE, "feature")      # no planes to take the statistic of
            if auto and a["host"] and not self.planes_valid:
                return Outcome(PT_ERR_STATE, "feature")      # the host layer reads the planes first
            if not self.whole_frame:
                return Outcome(PT_ERR_ARG, "whole frame")
            if not self.planes_valid:
                return Outcome(PT_ERR_STATE, "feature")
        return OK

    def apply(self, op, camera=None):
        """The outcome of the call; on success the flags move."""
        out = self.outcome(op)
        if out.code != PT_OK:
            return out
        k, a = op.kind, op.args
        if k == "render":                    # Pathtracer::renderChunks, then pt_render
            self.made_adaptive = self.denoised = False
            self.frames = (0 if a["ignore"] else self.frames) + a["chunks"]
            self.counts_valid = self.moments_valid = False
        elif k == "render_raw":              # pt_render alone: no frame accounting, the host flags stay
            self.counts_valid = self.moments_valid = False
        elif k == "adaptive":
            self.made_adaptive, self.denoised, self.frames = True, False, 0
            self.counts_valid = self.moments_valid = True
        elif k == "features":
            self.planes_valid, self.planes_camera, self.planes_read = True, camera, True
        elif k == "denoise":
            self.denoised_valid = True
            if a["host"]:
                self.denoised = True
        elif k == "rng":                     # pt_write_rng: the streams are no longer the moments'
            self.moments_valid = False
        elif k == "scene":                   # Pathtracer::setScene (+ pt_set_texture, pt_set_skybox of the loader)
            self.denoised = False
            self.moments_valid = self.planes_valid = False
        elif k == "texture":                 # pt_set_texture on the context: the host layer does not see it
            self.moments_valid = self.planes_valid = False
        elif k == "variant":
            self.variant = a["variant"]
        elif k == "run_ahead":
            self.run_ahead = a["mode"]
        elif k == "groups":
            self.groups = a["mode"]
        return out


# ------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------
def pair_circuit():
    """An Euler circuit of the complete directed graph over KINDS with loops (Hierholzer, fixed shuffle):
    170 kinds in which every ordered pair of kinds is adjacent exactly once."""
    rnd = random.Random(20261020)
    n = len(KINDS)
    out = {u: rnd.sample(range(n), n) for u in range(n)}
    stack, circuit = [0], []
    while stack:
        u = stack[-1]
        if out[u]:
            stack.append(out[u].pop())
        else:
            circuit.append(stack.pop())
    return [KINDS[u] for u in reversed(circuit)]


def named_blocks():
    """The sequences the issue names, as blocks of (kind, forced arguments)."""
    blocks = []
    for inv in ("camera", "rng", "scene", "texture", "adaptive"):        # stash-making render -> inv -> render
        blocks.append([("variant", {"variant": 0}), ("run_ahead", {"mode": 2}), ("render", {"spp": 4, "ignore": True}),
                       (inv, {"reset": True} if inv == "adaptive" else {}),
                       ("render", {"spp": 4, "ignore": inv == "adaptive"})])
    for inv in ("rng", "scene", "texture", "render_raw", "render"):     # adaptive -> inv -> adaptive(reset = False)
        blocks.append([("variant", {"variant": 0}), ("adaptive", {"reset": True}),
                       (inv, {"ignore": True} if inv == "render" else {}), ("adaptive", {"reset": False})])
    for inv in ("scene", "texture"):                                    # features -> scene change -> denoise
        blocks.append([("features", {}), (inv, {}), ("denoise", {})])
    blocks.append([("groups", {"mode": 2}), ("render", {}), ("groups", {"mode": 1}), ("render", {}),
                   ("groups", {"mode": 4}), ("render", {})])
    return blocks


def draw(kind, rnd, model, forced):
    """Seeded arguments of one call, every one inside the documented accepted range."""
    if kind in ("render", "render_raw"):
        a = {"spp": rnd.choice((1, 2, 4)), "chunks": rnd.choice((1, 2, 3)), "ignore": rnd.random() < 0.5}
        if kind == "render" and model.adaptive and rnd.random() < 0.8:
            a["ignore"] = True
    elif kind == "adaptive":
        can = model.adaptive and model.moments_valid
        a = {"spp": rnd.choice((2, 4)), "min_calls": 2, "max_calls": rnd.choice((3, 4, 6)),
             "tolerance": rnd.choice((0.0, 0.2, 1e9)), "reset": not (rnd.random() < (0.5 if can else 0.15))}
    elif kind == "denoise":
        a = {"sigma": rnd.choice((DENOISE_SIGMA, None)), "host": rnd.random() < 0.5}
    elif kind == "camera":
        a = {"how": rnd.choice(("rotate", "translate")), "x": round(rnd.uniform(-0.05, 0.05), 3),
             "y": round(rnd.uniform(-0.05, 0.05), 3), "z": round(rnd.uniform(-0.05, 0.05), 3)}
    elif kind == "scene":
        a = {"name": rnd.choice(SCENES)}
    elif kind == "texture":
        a = {"slot": rnd.randrange(8), "texel": rnd.choice(TEXELS)}
    elif kind == "variant":
        a = {"variant": rnd.choice((0, 0, 0) + ADAPTIVE_VARIANTS + SHIPPED_VARIANTS)}
    elif kind == "run_ahead":
        a = {"mode": rnd.randrange(4)}
    elif kind == "groups":
        a = {"mode": rnd.choice((0, 1, 2, 4))}
    elif kind == "knob":
        which = rnd.choice(sorted(KNOBS))
        a = {"which": which, "value": rnd.choice(KNOBS[which])}
    else:                                    # features, rng
        a = {}
    a.update(forced)
    return a


def whole_frame_blocks():
    """Named sequences whose denoise must run: for walks on a context that holds the whole frame."""
    blocks = [[("variant", {"variant": 0}), ("adaptive", {"reset": True}), (inv, {}), ("features", {}), ("denoise", {})]
              for inv in ("scene", "texture", "rng")]       # the counts must still divide (pt_denoise after a change)
    blocks.append([("features", {}), ("denoise", {"host": True}), ("scene", {})])   # a scene load ends "denoised"
    return blocks


def pair_counts(first, first_out, second, second_out):
    """An adjacent pair exercises a transition when its first call ran, and its second too unless the first is
    what makes it refuse (a scene or texture change before a denoise: the planes are void by contract)."""
    inherent = first in ("scene", "texture") and second == "denoise"
    return first_out.code == PT_OK and (second_out.code == PT_OK or inherent)


class _Walk:
    """One seed's walk while it is being built: its random stream, the model along it, the calls so far."""

    def __init__(self, seed):
        self.seed, self.rnd = seed, random.Random(seed)
        self.whole = CONFIGS[seed].band_rows == 1
        self.model = Model(self.whole)
        self.ops, self.outs = [], []

    def extend(self, plan, must=False):
        """Append calls; with `must` their arguments are forced to ones the model accepts in its state then."""
        for i, (kind, forced) in enumerate(plan):
            if must:
                nxt = plan[i + 1][0] if i + 1 < len(plan) else None
                forced = dict(self.accepted(kind, nxt), **forced)
            op = Op(kind, draw(kind, self.rnd, self.model, forced))
            self.outs.append(self.model.apply(op))
            self.ops.append(op)

    def accepted(self, kind, nxt):
        if kind == "render" and self.model.adaptive:
            return {"ignore": True}
        if kind == "adaptive":
            return {"reset": True}
        if kind == "variant" and nxt == "adaptive":
            return {"variant": 0}
        return {}

    def pairs(self):
        return {(p.kind, q.kind) for p, q, a, b in zip(self.ops, self.ops[1:], self.outs, self.outs[1:])
                if pair_counts(p.kind, a, q.kind, b)}

    def repair(self, first, second):
        """Calls that put the model where `first` and then `second` run, then the two."""
        prep = []
        if "adaptive" in (first, second) and first != "variant" and self.model.variant not in ADAPTIVE_VARIANTS:
            prep.append(("variant", {"variant": 0}))
        if "denoise" in (first, second) and first != "features" and not self.model.planes_valid:
            prep.append(("features", {}))
        self.extend(prep + [(first, {}), (second, {})], must=True)


def build_walks():
    """The walks of SEEDS, {seed: calls}.  Each is its slice of the pair circuit, its share of the named blocks,
    the repairs, then seeded filler up to STEPS.  They are built together because the repairs close what all
    of them together leave open: every ordered pair of kinds that does not yet occur as pair_counts asks gets
    a short block of its own, on the shortest walk that can run it."""
    parts = len(SEEDS)
    walks = {s % parts: _Walk(s) for s in SEEDS}
    circuit = pair_circuit()
    edges = len(circuit) - 1
    per = -(-edges // parts)
    for part, w in walks.items():
        kinds = circuit[part * per:min(edges, (part + 1) * per) + 1]
        for j, k in enumerate(kinds):
            # a denoise should usually find planes: where it or its successor is one and nothing void them in
            # between, make them first (the pair this splits is closed by the repairs if it occurs nowhere else)
            before, after = kinds[j - 1] if j else None, kinds[j + 1] if j + 1 < len(kinds) else None
            wanted = (k == "denoise" and before not in ("scene", "texture")) or \
                     (after == "denoise" and k not in ("scene", "texture", "features"))
            if w.whole and wanted and not w.model.planes_valid:
                w.extend([("features", {})])
            w.extend([(k, {})])
        for i, block in enumerate(named_blocks()):
            if i % parts == part:
                w.extend(block)
    whole = [w for w in walks.values() if w.whole]
    small = min(whole, key=lambda w: CONFIGS[w.seed].width)

    def shortest(ws):
        return min(ws, key=lambda w: (len(w.ops), w.seed))
    for i, block in enumerate(whole_frame_blocks()):
        (small if i == 0 else shortest(whole)).extend(block, must=True)     # the smallest frame denoises too
    for first in KINDS:
        for second in KINDS:
            if not any((first, second) in w.pairs() for w in walks.values()):
                shortest(whole if "denoise" in (first, second) else list(walks.values())).repair(first, second)
    for w in walks.values():
        while len(w.ops) < STEPS:
            w.extend([(w.rnd.choice(KINDS), {})])
    return {w.seed: w.ops for w in walks.values()}


_walks = {}


def generate(seed):
    """The walk of one of SEEDS (build_walks, built once)."""
    if not _walks:
        _walks.update(build_walks())
    return list(_walks[seed])


# ------------------------------------------------------------------------------------------------
# the oracle's side
# ------------------------------------------------------------------------------------------------
class OracleWalk:
    """What the reference's Pathtracer holds, call after call: the accumulation, the XORWOW states, the
    camera, the scene with every texture ever loaded (handles grow across loads) and the sky handle (a scene
    without a sky leaves the last one set, SceneLoader.cpp), and the moments of an adaptive render."""

    def __init__(self, scenes_dir, config, scene=START_SCENE):
        self.dir, self.cfg = scenes_dir, config
        self.textures, self.skybox = [], 0
        self.camera = None
        self.scene = self.load(scene)
        c = config
        self.ref = po.OracleRenderer(self.scene, c.width, c.height, c.row_offset, c.row_stride, band_rows=c.band_rows)
        self.accum = self.ref.accum.copy()
        self.ad = None
        self.planes_scene = self.planes_camera = None

    def load(self, name):
        L = po.lib()
        path = self.dir / f"{name}.scene.json"
        si = po.parse_scene(path)
        base = len(self.textures)
        self.textures.extend(si.textures)
        cpu = []
        for i in range(len(si)):
            handle = si.texture_handles[i] + base if si.texture_handles[i] else 0
            mat = po.Material()
            L.or_material_make(si.material_types[i], po.f3(si.base_colors[i]), po.f3(si.emissives[i]), si.roughness[i],
                               si.metalness[i], handle, C.byref(mat))
            h = po.CpuHittable()
            L.or_cpu_hittable_make(si.types[i], po.f3(si.positions[i]), po.f3(si.rotations[i]), po.f3(si.scales[i]),
                                   C.byref(mat), C.byref(h))
            cpu.append(h)
        sc = po.OracleScene()
        sc.textures = self.textures              # the same list: a texture call reaches every scene
        sc.cpu = cpu
        sc.set_scene(cpu)
        if isinstance(json.loads(path.read_text()).get("skybox"), str):
            self.skybox = si.skybox + base if si.skybox else 0
        sc.skybox = self.skybox
        L.or_camera_make(po.f3(si.camera_position), po.f3(si.camera_look_at), po.f3([0.0, 1.0, 0.0]), si.camera_fovy,
                         po.aspect_of(self.cfg.width, self.cfg.height), C.byref(sc.camera))
        self.camera = sc.camera
        return sc

    def texture_handle(self, slot):
        return 1 + slot % len(self.textures)

    def apply(self, op):
        """Mirror a call that succeeded."""
        k, a = op.kind, op.args
        if k in ("render", "render_raw"):
            self.ref.accum[:] = self.accum
            self.ref.render(self.camera, a["spp"], a["ignore"], chunks=a["chunks"])
            self.accum = self.ref.accum.copy()
        elif k == "adaptive":
            if a["reset"]:
                self.ad = AdaptiveOracle(self.ref)
            self.ad.render(self.camera, a["spp"], a["min_calls"], a["max_calls"], a["tolerance"], ADAPTIVE_FLOOR, a["reset"])
            self.accum = self.ad.accum.copy()
        elif k == "features":
            self.planes_scene, self.planes_camera = self.scene, po.Camera.from_buffer_copy(bytes(self.camera))
        elif k == "camera":
            fn = po.lib().or_camera_rotate if a["how"] == "rotate" else po.lib().or_camera_translate
            fn(C.byref(self.camera), a["x"], a["y"], a["z"])
        elif k == "scene":
            self.scene = self.ref.scene = self.load(a["name"])
        elif k == "texture":
            self.textures[self.texture_handle(a["slot"]) - 1] = np.tile(np.array(a["texel"], dtype=F), (4, 4, 1))

    def rng_array(self):
        return self.ref.rng_array()

    def first_hit(self):
        """Of the last features call: (primitive index or 0xffffffff, hit, emissive) per pixel."""
        osc, c = self.planes_scene, self.cfg
        n = osc.prim_count
        ids = first_hits(osc, [(i + 1, 0, 0) for i in range(n)], c.width, c.height, (c.band_rows, c.row_offset, c.row_stride),
                         camera=self.planes_camera)[..., 0]
        hit = ids > 0
        prim = np.where(hit, ids.astype(np.int64) - 1, 0xffffffff).astype(np.uint32)
        em = np.array([any(v != 0 for v in osc.prims[i].mat.emissive) for i in range(n)])
        return prim, hit, hit & em[np.where(hit, prim, 0)]

    def image(self, how, frames):
        """getHDRImageData / getImageData of the accumulation: (float32 x 4, RGBA8)."""
        a = np.ascontiguousarray(self.accum)
        npix = a.shape[0] * a.shape[1]
        ldr = np.zeros(a.shape[:2] + (4,), dtype=np.uint8)
        if how == "frames":
            hdr = np.zeros_like(a)
            po.lib().or_hdr_normalize(po.fptr(a), npix, frames, po.fptr(hdr))
            po.lib().or_tonemap(po.fptr(a), npix, frames, ldr.ctypes.data_as(C.POINTER(C.c_uint8)))
            return hdr, ldr
        n = self.ad.n
        with np.errstate(all="ignore"):
            hdr = a / np.maximum(n, 1).astype(F)[..., None]
        one = np.zeros_like(ldr)
        for k in np.unique(n):               # the oracle's tonemap with frames = n, once per distinct n
            po.lib().or_tonemap(po.fptr(a), npix, int(k), one.ctypes.data_as(C.POINTER(C.c_uint8)))
            ldr[n == k] = one[n == k]
        return hdr, ldr

    @staticmethod
    def tonemap_denoised(out):
        """pt_tonemap's arithmetic with divisor 1."""
        o = np.ascontiguousarray(out, dtype=F)
        ldr = np.zeros(o.shape[:2] + (4,), dtype=np.uint8)
        po.lib().or_tonemap(po.fptr(o), o.shape[0] * o.shape[1], 1, ldr.ctypes.data_as(C.POINTER(C.c_uint8)))
        return ldr

    @staticmethod
    def denoise(color, planes, sigma):
        d = DENOISE
        flags = (dm.DEMODULATE if d["demodulate"] else 0) | (dm.SAME_PRIMITIVE if d["same_primitive"] else 0)
        return dm.model(color, *planes, d["iterations"], sigma, d["sigma_plane"], d["normal_power_log2"], flags)
