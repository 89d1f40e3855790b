"""Speculative sample groups on synthetic streams: a toy sample stream, its serial truth,
and numpy restatements of the three device stages -- ssg_guess_kernel (csrc/pt_dev_fold.h), ssg_load /
ssg_finish (csrc/pt_dev_groups.h) and ssg_fold_kernel -- for tests/test_ssg_model.py (CPU) and
tests/test_gpu_ssg_stages.py (the same inputs through pathtracercuda_amd/lib/ssg_stages on the GPU).

A pixel's samples are one stream: "a sample that starts at draw-pair offset o of pixel p takes len(p, o)
pairs and returns colour(p, o)".  The fold of any consistent set of logs must equal the serial fold, so the
truth needs no ray tracing.  The lane model takes a SCHEDULE (which item of a tile logs its next sample), so
the window bits a lane sees are a test input.  Every index the lane and fold models form into a log, window,
start or fold array is checked against the array's extent (chk); numpy's wrapping negative indices are never
relied on.  REGIONS names the paths whose reach the tests assert, counted in pixels."""
import collections
import dataclasses

import numpy as np

from oracle import pyoracle

F_ACC, F_COL, F_SC, F_DONE, F_OFF, F_H, F_ST, F_FLAG, F_ODD, F_SQ, FOLD_WORDS = 0, 3, 6, 7, 8, 9, 10, 16, 17, 18, 19
START_WORDS, FOLD_BATCH, WIN_WORDS, IDLE = 8, 16, 16, 0xFFFFFFFF
M32 = 0xFFFFFFFF

REGIONS = (
    "join A at w == 0", "join A at w == win*64 - 1", "join A at w % 64 == 0, w >= 64",
    "join B at off == hStart + win*64", "join refused: kh == ch", "second-phase fall-back",
    "h advanced by the window rule", "h advanced by the latest-group rule",
    "batch cut by a phase-A bit", "batch cut by a phase-B bit", "batch cut by pos >= hNext", "batch cut by w > window",
    "batch of exactly 16", "last batch of 1", "call boundary inside a batch", "log ends at cap",
    "dead end in round 0", "dead end again in round 1", "finished in round >= 2", "done == total inside a patch log",
    "last group stopped by stopOff", "lane outside the image", "pos >= ssgTiles",
)

# one-token changes of the device text, restated (tests/test_ssg_model.py shows each one fails)
FOLD_MUTATIONS = ("ignore_c0", "fold_every", "state_plus2", "popc_mask", "join_nobit", "win_ge", "prevrel0", "h_one",
                  "fallback_base")
GUESS_MUTATIONS = ("bump_lt", "no_half", "m_ge", "podd_le", "phaseB_skip1")
MUT = set()        # the mutations in force (test use only)


class Bounds(AssertionError):
    """An index outside its array: the device would read or write out of range."""


def chk(ok, what):
    if not np.all(ok):
        raise Bounds(what)


# ---- the toy stream ------------------------------------------------------------------------------------
# classes: 0 always 1 (sky), 1 always 2, 2: 2 or 4 with ~1 % threes, 3 always 3, 4 always 6, 5 uniform 1..6,
# 6: 1 or 2 (mean 1.5), 7: 6, but every parse is brought onto offsets s0 and s1 (a sample starting within
# six pairs before one ends there): the directed class that puts a junction on a chosen window position
def _u32(x):
    return np.asarray(x, dtype=np.uint32)


def _mix(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def toy_hash(seed, o):
    return _mix(_u32(seed) ^ (_u32(o) * np.uint32(0x9E3779B1)))


def toy_len(seed, cls, s0, s1, o):
    o = _u32(o)
    h = toy_hash(seed, o)
    two4 = np.where(h % np.uint32(100) == 0, 3, np.where((h >> np.uint32(8)) & np.uint32(1), 4, 2))
    L = np.choose(np.minimum(cls, 7), [1, 2, two4, 3, 6, 1 + h % np.uint32(6), 1 + ((h >> np.uint32(8)) & np.uint32(1)), 6])
    L = _u32(L)
    for s in (s1, s0):
        s = _u32(s)
        near = (cls == 7) & (o < s) & (s - o <= np.uint32(6))
        L = np.where(near, s - o, L)
    return _u32(L)


def toy_colour(seed, o):
    """Three finite floats, magnitude 2^-12 .. 2^12, either sign: [..., 3] float32."""
    h = toy_hash(seed, o)
    out = np.empty(h.shape + (3,), dtype=np.uint32)
    for ch in range(3):
        g = _mix(h + np.uint32(((ch + 1) * 0x632BE5AB) & M32))
        e = np.uint32(115) + ((g >> np.uint32(23)) & np.uint32(0xFF)) % np.uint32(25)
        out[..., ch] = (g & np.uint32(0x807FFFFF)) | (e << np.uint32(23))
    return out.view(np.float32)


# ---- cases ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Case:
    name: str
    G: int
    spp: int
    chunks: int
    ignore: int = 0
    width: int = 13
    height: int = 10
    order: tuple = (0x00010001, 0x00000000, 0x00010000, 0x00000001)     # a permutation of the 2 x 2 tiles
    tiles: int = 4                  # ssgTiles
    look: tuple = (64, 16)
    classes: tuple = tuple(range(7))    # dealt to the pixels in seeded order
    stats: str = "truth"            # pairs input: "truth" (what a fold of this stream measures), "default"
                                    # (none: 2.0, -1.0, 1.0) or "mixed" (truth, a quarter of the pixels default)
    directed: tuple = ()            # class 7 pixels, dealt in turn: (group h, w) -> s0 = 3, s1 = hStart(h) + w under
                                    # the statistics (6, 0, 0); or ("abs", s0, s1, m, podd, var)
    seed: int = 1

    @property
    def total(self):
        return self.spp * self.chunks

    @property
    def n(self):
        return self.total // self.G

    @property
    def cap(self):
        return min(self.total, 2 * self.n + 64, 10000)

    @property
    def win(self):
        return (self.n * 6 + 256 + 63) // 64 if self.G == 2 else WIN_WORDS

    @property
    def J(self):
        return 2 * self.G - 1

    @property
    def tilesX(self):
        return (self.width + 7) // 8

    @property
    def tilesY(self):
        return (self.height + 7) // 8

    @property
    def npix(self):
        return self.width * self.height

    @property
    def threads(self):
        return (self.tiles * 64 + 255) // 256 * 256


def cases():
    d = (((1, 1023), (1, 1024), (1, 64), (1, 640), (2, 1023), (1, 1025)))
    return [
        Case("g2_33", 2, 3, 11, ignore=1, stats="mixed"),
        Case("g3_64", 3, 8, 8, ignore=0),
        Case("g5_1001", 5, 7, 143, ignore=1, classes=(1, 2, 4, 4, 5, 7, 7, 7), directed=d, stats="mixed"),
        # class 7 here: default statistics put the last group at 224 with stopOff 291, so its first phase logs
        # 12 samples and ends at 296; the true parse (onto residue 4, through groups 2 and 5) first meets it
        # there, at a start from which nothing was logged: the join is refused (kh == ch)
        Case("g8_128", 8, 8, 16, ignore=0, tiles=3, stats="mixed", classes=tuple(range(8)),
             directed=(("abs", 4, 296, 2.0, -1.0, 1.0),)),
        Case("g4_64", 4, 1, 64, ignore=1),
        Case("g2_2", 2, 1, 2, ignore=0, stats="default"),
    ]


def big_case():
    """10,000 six-pair samples in group 0's item of one tile: the default statistics put group 1 at 10000 and
    10001, which no six-pair parse from 0 meets, so item 0 runs to cap = 10000 samples and its 16-bit end
    offsets to their documented bound, 60,000."""
    return Case("g2_10000", 2, 100, 100, ignore=0, width=8, height=8, order=(0,), tiles=1, classes=(4,), stats="default")


class Pixels:
    """Per-pixel inputs of a case: XORWOW seed, toy seed and class, start accumulation value, statistics."""

    def __init__(self, cs):
        r = np.random.default_rng(cs.seed * 7919 + 17)
        n = cs.npix
        self.seed64 = r.integers(0, 2**63, n, dtype=np.uint64)
        self.tseed = r.integers(0, 2**32, n, dtype=np.uint32)
        self.cls = np.asarray(cs.classes, dtype=np.uint32)[r.permutation(n) % len(cs.classes)]
        self.s0 = np.zeros(n, dtype=np.uint32)
        self.s1 = np.zeros(n, dtype=np.uint32)
        self.accum0 = np.concatenate([toy_colour(self.tseed ^ np.uint32(0x5bd1e995), np.arange(n, dtype=np.uint32)),
                                      np.ones((n, 1), np.float32)], axis=1)
        self.rng0 = pyoracle.dev_xorwow_skip(self.seed64, np.zeros(n, np.uint32)).T.copy()      # [6][npix]
        self._states = {}
        self.pairs = None if cs.stats == "default" else self._stats(cs, r)
        if cs.directed:          # the directed pixels' junctions, from the guess this case will make
            idx = np.flatnonzero(self.cls == 7)
            ent = [cs.directed[i % len(cs.directed)] for i in range(len(idx))]
            for li, e in zip(idx, ent):       # statistics: six even pairs, or the entry's own
                self.pairs[:, li] = e[3:] if e[0] == "abs" else (6.0, 0.0, 0.0)
            offs = guess_offsets(cs, self.pairs)
            for li, e in zip(idx, ent):
                if e[0] == "abs":             # ("abs", s0, s1, m, podd, var)
                    self.s0[li], self.s1[li] = e[1], e[2]
                else:                         # (h, w): off residue 0 and 1 mod 6, then onto hStart(h) + w
                    self.s0[li], self.s1[li] = 3, offs[e[0] - 1][li] + e[1]

    def _stats(self, cs, r):
        # what a fold measures on this stream: mean, odd fraction and variance of the first `total` lengths
        tr_len = stream_lengths(self, cs.total)
        mean = tr_len.mean(axis=0, dtype=np.float64).astype(np.float32)
        odd = (tr_len & 1).mean(axis=0, dtype=np.float64).astype(np.float32)
        var = tr_len.var(axis=0, dtype=np.float64).astype(np.float32)
        p = np.stack([mean, odd, var])
        if cs.stats == "mixed":
            dflt = r.random(cs.npix) < 0.25
            p[0][dflt], p[1][dflt], p[2][dflt] = 2.0, -1.0, 1.0
        return p

    def state(self, li, off):
        """The pixel's XORWOW state 2 * off draws after its start state: [6] words."""
        key = (int(li), int(off))
        if key not in self._states:
            self._states[key] = pyoracle.dev_xorwow_skip(self.seed64[li:li + 1], np.asarray([2 * int(off)], np.uint32))[0]
        return self._states[key]

    def states(self, li, off):
        li, off = np.asarray(li), np.asarray(off)
        return pyoracle.dev_xorwow_skip(self.seed64[li.ravel()], (2 * off.ravel().astype(np.uint64)).astype(np.uint32))


def stream_lengths(px, count):
    """[count][npix] lengths of the first `count` samples of every pixel's true parse."""
    o = np.zeros(px.tseed.size, dtype=np.uint32)
    out = np.empty((count, o.size), dtype=np.uint32)
    for i in range(count):
        out[i] = toy_len(px.tseed, px.cls, px.s0, px.s1, o)
        o = o + out[i]
    return out


class Truth:
    """The serial fold: after d samples of every pixel, as ssg_fold_kernel's sums do it (color += c; at spp
    acc = color + acc, or color on the first call with ignoreFirst)."""

    def __init__(self, cs, px):
        self.cs, self.px = cs, px
        n, T = cs.npix, cs.total
        self.lens = stream_lengths(px, T)
        self.off = np.zeros((T + 1, n), dtype=np.uint32)
        self.off[1:] = np.cumsum(self.lens, axis=0, dtype=np.uint64).astype(np.uint32)
        self.acc = np.empty((T + 1, n, 3), np.float32)
        self.col = np.empty((T + 1, n, 3), np.float32)
        acc = np.zeros((n, 3), np.float32) if cs.ignore else px.accum0[:, :3].copy()
        col = np.zeros((n, 3), np.float32)
        self.acc[0], self.col[0] = acc, col
        for d in range(T):
            col = col + toy_colour(px.tseed, self.off[d])
            if (d + 1) % cs.spp == 0:
                acc = col.copy() if (d + 1 == cs.spp and cs.ignore) else col + acc
                col = np.zeros((n, 3), np.float32)
            self.acc[d + 1], self.col[d + 1] = acc, col

    def at(self, li, d):
        return dict(acc=self.acc[d, li], col=self.col[d, li], sc=(d % self.cs.spp) | ((d // self.cs.spp) << 16),
                    off=int(self.off[d, li]), st=self.px.state(li, self.off[d, li]))


def pixel_map(cs):
    """li[pos][lane] (-1: no pixel) for the threads the guess and fold kernels launch, and the region counts."""
    li = np.full((cs.threads // 64, 64), -1, dtype=np.int64)
    reg = collections.Counter()
    for pos in range(cs.threads // 64):
        if pos >= cs.tiles:
            reg["pos >= ssgTiles"] += 64
            continue
        chk(pos < len(cs.order), "order index")
        t = cs.order[pos]
        tx, ty = t & 0xFFFF, t >> 16
        for lane in range(64):
            x, y = tx * 8 + (lane & 7), ty * 8 + (lane >> 3)
            if ty < cs.tilesY and x < cs.width and y < cs.height:
                li[pos, lane] = y * cs.width + x
            else:
                reg["lane outside the image"] += 1
    return li[:cs.tiles], reg


# ---- the guess -----------------------------------------------------------------------------------------
def _guess_fields(cs, pairs, npix):
    f = np.float32
    if pairs is None:
        m, podd, var = np.full(npix, 2.0, f), np.full(npix, -1.0, f), np.full(npix, 1.0, f)
    else:
        m, podd = pairs[0].astype(f), pairs[1].astype(f)
        var = np.where(podd >= f(0), pairs[2].astype(f), f(1.0))
    with np.errstate(invalid="ignore"):
        m = np.where(m >= f(1.0), np.fmin(m, f(6.0)), f(1.0)).astype(f)
        total = f(cs.total)
        stop = (total * m + f(3.0) * np.sqrt(total * np.fmax(var, f(0.05))) + f(2.0)).astype(f)
        podd_lt = (podd <= f(0.06)) if "podd_le" in MUT else (podd < f(0.06))
        stable = np.where(podd >= f(0), podd_lt, np.abs(m - f(2.0)) < f(0.25))
        q = np.where(stable, f(2.0), np.rint(m)).astype(f)
        lattice = stable | ((q >= f(3.0)) & (np.abs(m - q) < f(0.02)))
        dual = stable & ((m >= f(1.5)) if "m_ge" in MUT else (m > f(1.5)))
    return m, q, lattice, dual, stop.astype(np.uint32)


def guess_offsets(cs, pairs):
    """[G - 1][npix] start offsets of groups 1 .. G - 1 (phase A)."""
    f = np.float32
    npix = cs.npix if pairs is None else pairs.shape[1]
    m, q, lattice, dual, _ = _guess_fields(cs, pairs, npix)
    half = f(0.0) if "no_half" in MUT else f(0.5)
    off = np.zeros(npix, np.uint32)
    out = []
    for g in range(1, cs.G):
        gn = f(g * cs.n)
        a = q.astype(np.uint32) * (gn * (m / q) + half).astype(f).astype(np.uint32)
        b = (gn * m + f(0.5)).astype(f).astype(np.uint32)
        o = np.where(lattice, a, b).astype(np.uint32)
        bump = (o < off) if "bump_lt" in MUT else (o <= off)
        o = np.where(bump, off + np.uint32(1), o).astype(np.uint32)
        off = o
        out.append(o)
    return out


def guess(cs, px, pairs, lim=None, at=None):
    """Start records [items][8][64] as ssg_guess_kernel writes them into a zeroed buffer; at: the offset of
    every pixel's current state in its stream (a guess after a fold), else 0."""
    lim, _ = pixel_map(cs) if lim is None else (lim, None)
    at = np.zeros(cs.npix, np.uint32) if at is None else np.asarray(at, np.uint32)
    _, _, _, dual, stop = _guess_fields(cs, pairs, cs.npix)
    offs = guess_offsets(cs, pairs)
    start = np.zeros((cs.tiles * cs.J, START_WORDS, 64), np.uint32)
    pos, lane = np.nonzero(lim >= 0)
    li = lim[pos, lane]
    for g in range(1, cs.G):
        o = offs[g - 1][li]
        itA = pos * cs.J + 2 * g - 1
        chk(itA + 1 < start.shape[0], "start record")
        start[itA, 0, lane] = o
        start[itA, 1:7, lane] = px.states(li, at[li] + o)
        start[itA, 7, lane] = stop[li] if g + 1 == cs.G else IDLE
        d = dual[li]
        oB = o + np.uint32(1)
        drawsB = (2 * o + (1 if "phaseB_skip1" in MUT else 2)).astype(np.uint32)
        stB = pyoracle.dev_xorwow_skip(px.seed64[li], 2 * at[li] + drawsB)
        start[itA + 1, 0, lane] = np.where(d, oB, IDLE)
        for w in range(6):
            start[itA + 1, 1 + w, lane] = np.where(d, stB[:, w], 0)
        start[itA + 1, 7, lane] = np.where(d, stop[li] if g + 1 == cs.G else IDLE, 0)
    return start


def guess_grid():
    """[3][points]: m, podd and var at, one ulp below and one ulp above each branch constant (1.0, 6.0, 1.5 and
    2 -+ 0.25, q -+ 0.02 on m; 0.06 on podd; 0.05 on var), m < 1, > 6 and NaN, podd < 0 (unknown)."""
    f = np.float32

    def around(x):
        return [np.nextafter(f(x), f(-99)), f(x), np.nextafter(f(x), f(99))]
    m = around(1.0) + around(6.0) + around(1.5) + around(1.75) + around(2.25) + around(2.98) + around(3.02) + around(4.98) + \
        around(5.02) + [f(0.5), f(7.0), f(np.nan), f(2.0), f(2.5), f(2.6), f(3.0), f(0.0), f(-3.0)]
    podd = around(0.06) + [f(-1.0), f(0.0), f(0.5), f(1.0)]
    var = around(0.05) + [f(0.0), f(1.0), f(7.5)]
    return np.asarray([(a, b, c) for a in m for b in podd for c in var], f).T


GRID_CASES, GRID_IDS = [(5, 7, 143), (4, 1, 4), (2, 3, 11)], ["n200", "n1", "g2"]


def grid_case(G, spp, chunks):
    """(case, pixels, li) whose statistics are the grid: 56 x 48 pixels, 42 tiles in a seeded order."""
    grid = guess_grid()
    order = tuple(int(t) for t in np.random.default_rng(3).permutation([(y << 16) | x for y in range(6) for x in range(7)]))
    cs = Case("grid", G, spp, chunks, width=56, height=48, order=order, tiles=len(order), classes=(5,), stats="default")
    assert grid.shape[1] <= cs.npix
    px = Pixels(cs)
    px.pairs = np.tile(np.asarray([[2.0], [-1.0], [1.0]], np.float32), (1, cs.npix))
    px.pairs[:, :grid.shape[1]] = grid
    return cs, px, pixel_map(cs)[0]


# ---- the lanes -----------------------------------------------------------------------------------------
def sched_earliest(steps, alive, rnd):
    return int(np.flatnonzero(alive)[0])


def sched_latest(steps, alive, rnd):
    return int(np.flatnonzero(alive)[-1])


def sched_round_robin(steps, alive, rnd):
    j = np.flatnonzero(alive)
    return int(j[np.argmin(steps[j])])


def sched_random(steps, alive, rnd):
    return int(rnd.choice(np.flatnonzero(alive)))


def sched_lag(L):
    """Phase A (odd items) lags phase B by L samples."""
    def pick(steps, alive, rnd):
        j = np.flatnonzero(alive)
        return int(j[np.argmin(steps[j] + L * (j & 1))])
    return pick


SCHEDULES = {
    "earliest": (sched_earliest, None), "latest": (sched_latest, None), "round-robin": (sched_round_robin, None),
    "random": (sched_random, None), "lag8 look(0,0)": (sched_lag(8), (0, 0)), "lag1 look(1,0)": (sched_lag(1), (1, 0)),
    "lag40 look(32,8)": (sched_lag(40), (32, 8)),
}


@dataclasses.dataclass
class Logs:
    log: np.ndarray       # [items][cap][3][64] float32
    end: np.ndarray       # [items][cap][64] uint16
    count: np.ndarray     # [items][64] uint32
    bits: np.ndarray      # [items][win][64] uint64 (shared by the patch rounds, which only read it)


def _getbit(bits, item, w, lane, win, what):
    chk((item >= 0) & (item < bits.shape[0]) & (w // 64 < win), what)
    return ((bits[item, w // 64, lane] >> (w % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


def lanes(cs, px, lim, start, schedule, look=None, seed=0, fold=None, bits=None, reg=None):
    """ssg_load, then ssg_finish per sample, item by item as `schedule` picks them; fold != None: a patch round
    (one carrier per tile from the fold words, reading `bits`)."""
    look = cs.look if look is None else look
    reg = collections.Counter() if reg is None else reg
    patch = fold is not None
    T, J, G, cap, win64 = cs.tiles, (1 if patch else cs.J), cs.G, cs.cap, cs.win * 64
    nit = T * J
    L = Logs(np.zeros((nit, cap, 3, 64), np.float32), np.zeros((nit, cap, 64), np.uint16), np.zeros((nit, 64), np.uint32),
             np.zeros((T * cs.J, cs.win, 64), np.uint64) if bits is None else bits)
    rnd = np.random.default_rng(seed)
    valid = lim >= 0
    lis = np.where(valid, lim, 0)
    sh = (T, J, 64)
    cur, base, k, h = (np.zeros(sh, np.uint32) for _ in range(4))
    limit, stopOff, alive = np.zeros(sh, np.uint32), np.full(sh, IDLE, np.uint32), np.zeros(sh, bool)
    posA, laneA = np.meshgrid(np.arange(T), np.arange(64), indexing="ij")
    # ssg_load
    for j in range(J):
        if patch:
            flag = (fold[F_FLAG, lis] & 1).astype(bool) & valid
            base[:, j] = fold[F_OFF, lis]
            h[:, j] = np.where(flag, np.minimum(fold[F_H, lis], G), G)      # a finished pixel's words are stale
            limit[:, j] = np.where(flag, np.minimum(cap, cs.total - fold[F_DONE, lis]), 0)
            alive[:, j] = flag & (limit[:, j] > 0)
        else:
            g = (j + 1) >> 1
            it = posA * cs.J + j
            if g:
                chk(it < start.shape[0], "start record")
                so = start[it, 0, laneA]
                idle = (so == IDLE) | ~valid
                base[:, j] = np.where(idle, 0, so)
                p, l = np.nonzero(~idle)
                L.bits[p * cs.J + j, 0, l] |= np.uint64(1)
                if g + 1 == G:
                    stopOff[:, j] = start[it, 7, laneA]
            else:
                idle = ~valid
                if g + 1 == G:
                    stopOff[:, j] = start[it, 7, laneA]
            h[:, j] = g + 1
            limit[:, j] = np.where(idle, 0, cap)
            alive[:, j] = ~idle & (cap > 0)
        cur[:, j] = base[:, j]

    def start_of(p, hh, l):          # start offset of group hh's phase A (IDLE where hh >= G)
        it = p * cs.J + 2 * np.minimum(hh, G - 1).astype(np.int64) - 1
        chk((it >= 0) & (it < start.shape[0]), "start record of group h")
        return np.where(hh < G, start[it, 0, l], IDLE).astype(np.uint32)

    hStart = np.empty(sh, np.uint32)
    for j in range(J):
        hStart[:, j] = start_of(posA, h[:, j], laneA) if G > 1 else IDLE
    steps = np.zeros(J, np.int64)
    while alive.any():
        j = schedule(steps, alive.any(axis=(0, 2)), rnd)
        steps[j] += 1
        p, l = np.nonzero(alive[:, j])
        li = lim[p, l]
        o = cur[p, j, l]
        ln = toy_len(px.tseed[li], px.cls[li], px.s0[li], px.s1[li], o)
        e = o + ln
        rel = e - base[p, j, l]
        kk = k[p, j, l]
        item = p * J + j
        chk((kk < cap) & (item < nit), "log record")
        chk(rel <= 0xFFFF, "16-bit end offset")
        L.log[item, kk, :, l] = toy_colour(px.tseed[li], o)
        L.end[item, kk, l] = rel
        kk = kk + 1
        stop = kk >= limit[p, j, l]
        atcap = stop & (kk == cap)
        g = G if patch else (j + 1) >> 1
        bitem = p * cs.J + j
        if 1 <= g < G:
            s = rel < win64
            chk(bitem[s] < L.bits.shape[0], "window word")
            L.bits[bitem[s], rel[s] // 64, l[s]] |= np.uint64(1) << (rel[s] % 64).astype(np.uint64)
        byStop = ~stop & (e >= stopOff[p, j, l])
        stop = stop | byStop
        if j >= 2 and not (j & 1) and not patch:
            c = ~stop & (rel + 1 < win64)
            stop[c] = _getbit(L.bits, bitem[c] - 1, rel[c] + 1, l[c], cs.win, "phase A window (second phase)")
            for Lk in look:
                c = ~stop & (kk > Lk) if Lk else np.zeros_like(stop)
                if c.any():
                    chk((kk[c] - 1 - Lk >= 0) & (kk[c] - 1 - Lk < cap), "look-back record")
                    wb = L.end[item[c], kk[c] - 1 - Lk, l[c]].astype(np.uint32) + 1
                    inw = wb < win64
                    got = np.zeros(wb.shape, bool)
                    got[inw] = _getbit(L.bits, bitem[c][inw] - 1, wb[inw], l[c][inw], cs.win, "phase A window (look-back)")
                    stop[c] = got
        hh, hs = h[p, j, l], hStart[p, j, l]
        while True:
            adv = (hh < G) & (e.astype(np.int64) > hs.astype(np.int64) + win64)
            if not adv.any():
                break
            hh = np.where(adv, hh + 1, hh)
            hs = np.where(adv, start_of(p, hh, l), hs)
        while True:
            can = hh + 1 < G
            nx = start_of(p, np.where(can, hh + 1, G), l)
            adv = can & (e >= nx)
            if not adv.any():
                break
            hh = np.where(adv, hh + 1, hh)
            hs = np.where(adv, nx, hs)
        c = ~stop & (hh < G) & (e >= hs)
        if c.any():
            w = e[c] - hs[c]
            itA = p[c] * cs.J + 2 * hh[c].astype(np.int64) - 1
            got = np.zeros(w.shape, bool)
            a = w < win64
            got[a] = _getbit(L.bits, itA[a], w[a], l[c][a], cs.win, "group h window, phase A")
            b = ~got & (w >= 1)
            got[b] = _getbit(L.bits, itA[b] + 1, w[b] - 1, l[c][b], cs.win, "group h window, phase B")
            stop[c] = got
        h[p, j, l], hStart[p, j, l] = hh, hs
        k[p, j, l] = kk
        cur[p, j, l] = e
        alive[p, j, l] = ~stop
        reg["log ends at cap"] += int(atcap.sum())
        reg["last group stopped by stopOff"] += int(byStop.sum())
    for j in range(J):
        L.count[posA * J + j, laneA] = np.where(valid, k[:, j], 0)
    return L


# ---- the fold ------------------------------------------------------------------------------------------
@dataclasses.dataclass
class FoldState:
    accum: np.ndarray     # [npix][4] float32
    rng: np.ndarray       # [6][npix] uint32
    fold: np.ndarray      # [19][npix] uint32
    pairs: np.ndarray     # [3][npix] float32
    dead: int = 0

    def copy(self):
        return FoldState(self.accum.copy(), self.rng.copy(), self.fold.copy(), self.pairs.copy(), self.dead)


def fold_state(cs, px):
    p = px.pairs if px.pairs is not None else np.stack([np.full(cs.npix, v, np.float32) for v in (2.0, -1.0, 1.0)])
    return FoldState(px.accum0.copy(), px.rng0.copy(), np.zeros((FOLD_WORDS, cs.npix), np.uint32), p.copy())


def _popc(x):
    return bin(x).count("1")


def fold(cs, px, lim, start, L, S, rnd_, patch=None, reg=None):
    """ssg_fold_kernel, round rnd_, over the logs L (and the patch logs of this round); updates S in place."""
    reg = collections.Counter() if reg is None else reg
    G, J, cap, win, win64, total, spp = cs.G, cs.J, cs.cap, cs.win, cs.win * 64, cs.total, cs.spp
    f = np.float32
    S.dead = 0
    nst = start.shape[0]
    for pos in range(cs.tiles):
        item0 = pos * J
        for lane in range(64):
            li = int(lim[pos, lane])
            if li < 0:
                continue
            R = set()
            F = S.fold
            so = [int(start[item0 + j, 0, lane]) for j in range(J)]
            bitsL = [[int(x) for x in L.bits[item0 + j, :, lane]] for j in range(J)]
            cntL = [int(L.count[item0 + j, lane]) for j in range(J)]
            odd = prevRel = sq = 0
            if rnd_ == 0:
                acc = np.zeros(3, f) if cs.ignore else S.accum[li, :3].copy()
                color = np.zeros(3, f)
                sIdx = c = done = off = 0
                h, inPatch, cur, k, base, cnt = 1, False, 0, 0, 0, cntL[0]
            else:
                if not (F[F_FLAG, li] & 1):
                    continue
                acc = F[F_ACC:F_ACC + 3, li].copy().view(f)
                color = F[F_COL:F_COL + 3, li].copy().view(f)
                sc = int(F[F_SC, li])
                sIdx, c, done, off = sc & 0xFFFF, sc >> 16, int(F[F_DONE, li]), int(F[F_OFF, li])
                h = 1 if "h_one" in MUT else min(int(F[F_H, li]), G)
                odd, sq = int(F[F_ODD, li]), int(F[F_SQ, li])
                inPatch, cur, k, base = True, G, 0, off
                chk(pos < patch.count.shape[0], "patch count")
                cnt = int(patch.count[pos, lane])

            def sw(j):
                chk(0 <= item0 + j < nst and j < J, "start record")
                return so[j]

            def bit(j, w):
                chk(0 <= j < J and 0 <= w // 64 < win, "window word")
                return (bitsL[j][w // 64] >> (w % 64)) & 1

            def kh_of(j, w):
                mask = (1 << (w % 64)) if "popc_mask" in MUT else (1 << (w % 64)) - 1
                return _popc(bitsL[j][w // 64] & mask) + sum(_popc(bitsL[j][q]) for q in range(w // 64))

            def end_of(j, kk):
                chk(0 <= kk < cap and 0 <= j < J, "end offset record")
                return int(L.end[item0 + j, kk, lane])

            hStart = sw(2 * h - 1) if h < G else IDLE
            while done < total:
                while h < G and ((off >= hStart + win64) if "win_ge" in MUT else (off > hStart + win64)):
                    h += 1
                    hStart = sw(2 * h - 1) if h < G else IDLE
                    R.add("h advanced by the window rule")
                while h + 1 < G:
                    nx = sw(2 * h + 1)
                    if off < nx:
                        break
                    h += 1
                    hStart = nx
                    R.add("h advanced by the latest-group rule")
                if h < G and off >= hStart:
                    joined = False
                    for ph in range(2):
                        if joined:
                            break
                        j = 2 * h - 1 + ph
                        if off < hStart + ph:
                            continue
                        w = off - hStart - ph
                        if w >= win64:
                            continue
                        if "join_nobit" not in MUT and not bit(j, w):
                            continue
                        kh = kh_of(j, w)
                        ch = cntL[j]
                        if kh < ch:
                            inPatch, cur, k, base, cnt, joined = False, j, kh, hStart + ph, ch, True
                            prevRel = end_of(j, kh - 1) if kh and "prevrel0" not in MUT else 0
                            if ph == 0:
                                if w == 0:
                                    R.add("join A at w == 0")
                                if w == win64 - 1:
                                    R.add("join A at w == win*64 - 1")
                                if w % 64 == 0 and w >= 64:
                                    R.add("join A at w % 64 == 0, w >= 64")
                            elif off == hStart + win64:
                                R.add("join B at off == hStart + win*64")
                        else:
                            R.add("join refused: kh == ch")
                    if joined:
                        h += 1
                        hStart = sw(2 * h - 1) if h < G else IDLE
                        continue
                if k >= cnt and not inPatch and cur >= 2 and not (cur & 1):
                    j = cur - 1
                    w = (off - (base - 1)) & M32
                    if w < win64 and bit(j, w):
                        kh = kh_of(j, w)
                        ch = cntL[j]
                        if kh < ch:
                            cur -= 1
                            k = kh
                            if "fallback_base" not in MUT:
                                base -= 1
                            cnt = ch
                            prevRel = end_of(j, kh - 1) if kh else 0
                            R.add("second-phase fall-back")
                            continue
                if k >= cnt:
                    break
                m = min(cnt - k, total - done, FOLD_BATCH)
                if inPatch:
                    chk(pos < patch.count.shape[0] and k + m <= cap, "patch log record")
                    er = [int(x) for x in patch.end[pos, k:k + m, lane]]
                    cols = patch.log[pos, k:k + m, :, lane]
                else:
                    chk(0 <= cur < J and k + m <= cap, "log record")
                    er = [int(x) for x in L.end[item0 + cur, k:k + m, lane]]
                    cols = L.log[item0 + cur, k:k + m, :, lane]
                if h < G and m > 1 and base + er[m - 2] >= hStart:
                    jA = 2 * h - 1
                    chk(jA + 1 < J, "window of group h, phase B")
                    hNext = sw(2 * h + 1) if h + 1 < G else IDLE

                    def bitw(j, w):
                        return bit(j, w) if w // 64 < win else 0
                    for jj in range(m - 1):
                        p_ = base + er[jj]
                        if p_ < hStart:
                            continue
                        w = p_ - hStart
                        why = None
                        if w > win64:
                            why = "batch cut by w > window"
                        elif p_ >= hNext:
                            why = "batch cut by pos >= hNext"
                        elif w < win64 and bitw(jA, w):
                            why = "batch cut by a phase-A bit"
                        elif w >= 1 and bitw(jA + 1, w - 1):
                            why = "batch cut by a phase-B bit"
                        if why:
                            m = jj + 1
                            R.add(why)
                            break
                if m == FOLD_BATCH:
                    R.add("batch of exactly 16")
                if m == 1 and done + 1 == total:
                    R.add("last batch of 1")
                if m > 1 and sIdx + m > spp:
                    R.add("call boundary inside a batch")
                endRel = prevRel
                for jj in range(m):
                    dlt = (er[jj] - endRel) & M32
                    odd = (odd + (dlt & 1)) & M32
                    sq = (sq + dlt * dlt) & M32
                    endRel = er[jj]
                prevRel = endRel
                for jj in range(m):
                    color = color + cols[jj]
                    sIdx += 1
                    if sIdx == spp or "fold_every" in MUT:
                        acc = color.copy() if ((c == 0 or "ignore_c0" in MUT) and cs.ignore) else color + acc
                        color = np.zeros(3, f)
                        sIdx = 0
                        c += 1
                off = base + endRel
                k += m
                done += m
            # the exact state at off
            rel = (off - base) & M32
            chk(rel <= 0x20000, "state advance")
            if inPatch:
                st0off = int(F[F_OFF, li])
            elif cur == 0:
                st0off = 0
            else:
                st0off = sw(cur)
            st = px.state(li, st0off + rel + (1 if "state_plus2" in MUT else 0))
            S.rng[:, li] = st
            S.accum[li] = (acc[0], acc[1], acc[2], 1.0)
            if done == total:
                if done > 0:
                    mean = f(off) / f(done)
                    S.pairs[0, li] = mean
                    S.pairs[1, li] = f(odd) / f(done)
                    S.pairs[2, li] = max(f(f(sq) / f(done)) - f(mean * mean), f(0.0))
                F[F_FLAG, li] = rnd_ << 8
                if rnd_ >= 2:
                    R.add("finished in round >= 2")
                if inPatch:
                    R.add("done == total inside a patch log")
            else:
                if done > 0:
                    S.pairs[0, li] = f(off) / f(done)
                F[F_ACC:F_ACC + 3, li] = acc.view(np.uint32)
                F[F_COL:F_COL + 3, li] = color.view(np.uint32)
                F[F_SC, li] = sIdx | (c << 16)
                F[F_DONE, li], F[F_OFF, li], F[F_H, li], F[F_ODD, li], F[F_SQ, li] = done, off, h, odd, sq
                F[F_ST:F_ST + 6, li] = st
                F[F_FLAG, li] = 1
                S.dead += 1
                if rnd_ <= 1:
                    R.add("dead end in round 0" if rnd_ == 0 else "dead end again in round 1")
            for name in R:
                reg[name] += 1
    return S


def chain(cs, px, schedule, look=None, rounds=3, seed=0, reg=None, each=None):
    """guess -> lanes -> fold -> (patch lanes -> fold) x rounds, as run_groups sequences them.  each(r, S, L, P)
    sees every round's result."""
    reg = collections.Counter() if reg is None else reg
    lim, r0 = pixel_map(cs)
    reg.update(r0)
    start = guess(cs, px, px.pairs, lim)
    L = lanes(cs, px, lim, start, schedule, look, seed, reg=reg)
    S = fold_state(cs, px)
    fold(cs, px, lim, start, L, S, 0, reg=reg)
    out = [(start, L, None, S.copy())]
    if each:
        each(0, S, L, None)
    for r in range(1, rounds + 1):
        if S.dead == 0:
            break
        P = lanes(cs, px, lim, start, sched_earliest, look, seed, fold=S.fold, bits=L.bits, reg=reg)
        fold(cs, px, lim, start, L, S, r, patch=P, reg=reg)
        out.append((start, L, P, S.copy()))
        if each:
            each(r, S, L, P)
    return out


# ---- files of pathtracercuda_amd/lib/ssg_stages (tools/ssg_stages.hip) ----------------------------------
def write_case(d, cs, px, start=None, logs=None, state=None, patch=None, look=None):
    """The inputs of a case as the tool reads them; start / logs / state / patch: the stage inputs made here."""
    look = cs.look if look is None else look
    hdr = [cs.width, cs.height, cs.tiles, cs.G, cs.spp, cs.chunks, cs.ignore, cs.cap, cs.win, look[0], look[1],
           len(cs.order), 0 if px.pairs is None else 1]
    np.asarray(hdr, np.uint32).tofile(d / "case.hdr")
    np.asarray(cs.order, np.uint32).tofile(d / "order.in")
    S = fold_state(cs, px) if state is None else state
    S.rng.astype(np.uint32).tofile(d / "rng.in")
    S.accum.astype(np.float32).tofile(d / "accum.in")
    np.stack([px.tseed, px.cls, px.s0, px.s1]).astype(np.uint32).tofile(d / "toy.in")
    if px.pairs is not None:
        S.pairs.astype(np.float32).tofile(d / "pairs.in")
    if state is not None:
        S.fold.tofile(d / "fold.in")
    if start is not None:
        start.tofile(d / "start.in")
    if logs is not None:
        logs.log.tofile(d / "log.in")
        logs.end.tofile(d / "end.in")
        logs.bits.tofile(d / "bits.in")
        logs.count.tofile(d / "count.in")
    if patch is not None:
        patch.log.tofile(d / "patchlog.in")
        patch.end.tofile(d / "patchend.in")
        patch.count.tofile(d / "patchcount.in")


def read_out(d, cs, tag):
    """What `dump:tag` wrote: (start, Logs, patch Logs, FoldState)."""
    def rd(name, dt, shape):
        a = np.fromfile(d / f"{name}.{tag}.out", dtype=dt)
        assert a.size == int(np.prod(shape)), f"{name}.{tag}.out: {a.size} words, expected {shape}"
        return a.reshape(shape)
    it, T, cap = cs.tiles * cs.J, cs.tiles, cs.cap
    bits = rd("bits", np.uint64, (it, cs.win, 64))
    L = Logs(rd("log", np.float32, (it, cap, 3, 64)), rd("end", np.uint16, (it, cap, 64)), rd("count", np.uint32, (it, 64)), bits)
    P = Logs(rd("patchlog", np.float32, (T, cap, 3, 64)), rd("patchend", np.uint16, (T, cap, 64)),
             rd("patchcount", np.uint32, (T, 64)), bits)
    S = FoldState(rd("accum", np.float32, (cs.npix, 4)), rd("rng", np.uint32, (6, cs.npix)),
                  rd("fold", np.uint32, (FOLD_WORDS, cs.npix)), rd("pairs", np.float32, (3, cs.npix)),
                  int(rd("dead", np.uint32, (1,))[0]))
    return rd("start", np.uint32, (it, START_WORDS, 64)), L, P, S


def check_against_truth(cs, tr, lim, S, where):
    """The invariant: a finished pixel's accum and rng are the truth's at d = total, a dead end's saved words
    the truth's at d = F_DONE.  Returns the failures as text lines."""
    bad = []
    F = S.fold
    for pos in range(cs.tiles):
        for lane in range(64):
            li = int(lim[pos, lane])
            if li < 0:
                continue
            if F[F_FLAG, li] & 1:
                d = int(F[F_DONE, li])
                if d >= cs.total:
                    bad.append(f"{where}: pixel {li}: dead end with done = {d}")
                    continue
                t = tr.at(li, d)
                got = dict(acc=F[F_ACC:F_ACC + 3, li], col=F[F_COL:F_COL + 3, li], sc=F[F_SC, li], off=F[F_OFF, li],
                           st=F[F_ST:F_ST + 6, li])
                want = dict(acc=t["acc"].view(np.uint32), col=t["col"].view(np.uint32), sc=t["sc"], off=t["off"], st=t["st"])
            else:
                t = tr.at(li, cs.total)
                got = dict(accum=S.accum[li, :3].view(np.uint32), w=S.accum[li, 3], rng=S.rng[:, li])
                want = dict(accum=t["acc"].view(np.uint32), w=np.float32(1.0), rng=t["st"])
            for key in got:
                if not np.array_equal(np.asarray(got[key]), np.asarray(want[key])):
                    bad.append(f"{where}: pixel {li} (class {int(tr.px.cls[li])}, "
                               f"{'dead end' if F[F_FLAG, li] & 1 else 'finished'}): {key} = {got[key]}, truth {want[key]}")
    return bad


# ---- the runs both test modules share (computed once) ---------------------------------------------------
ROUNDS = 3
_CACHE = {}


def case_named(name):
    return {c.name: c for c in cases() + [big_case()]}[name]


def schedules_of(name):
    return ("earliest",) if name == "g2_10000" else tuple(SCHEDULES)


def inputs(name):
    """(case, pixels, truth, li[pos][lane]) of a case, unchanged by its users."""
    if ("in", name) not in _CACHE:
        cs = case_named(name)
        px = Pixels(cs)
        _CACHE["in", name] = (cs, px, Truth(cs, px), pixel_map(cs)[0])
    return _CACHE["in", name]


def run(name, sched):
    """The model's chain of a case under a schedule: (rounds as chain() returns them, region counts)."""
    if (name, sched) not in _CACHE:
        cs, px, _, _ = inputs(name)
        pick, look = SCHEDULES[sched]
        reg = collections.Counter()
        _CACHE[name, sched] = (chain(cs, px, pick, look, ROUNDS, seed=5, reg=reg), reg)
    return _CACHE[name, sched]
