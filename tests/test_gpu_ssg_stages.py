"""The guess, lane and fold code of speculative sample groups, stage by stage, on the GPU.
pathtracercuda_amd/lib/ssg_stages (tools/ssg_stages.hip) runs the shipped ssg_guess_kernel, ssg_load /
ssg_finish and ssg_fold_kernel on the toy streams of tests/ssg_model.py, one child process per fixture:

  guess   the start records equal the model's word for word (a directed grid around every branch constant,
          and the statistics a fold has just written);
  fold    on the model's logs of every case and schedule, every word the fold writes equals the fold model's,
          round by round (the patch logs between the rounds too: a carrier reads fixed bits);
  lanes   the device's own logs depend on its scheduling, so they are held to the stream instead: every logged
          sample is the toy stream's at its offset, the window bits are exactly the logged starts, and every
          item stopped for a reason the rules allow;
  chain   guess -> lanes -> fold -> (patch -> fold) on the device alone: finished pixels equal the serial
          truth at d = total, dead ends at d = F_DONE.

The Python model runs every case first: a bounds assertion there fails the test before anything is launched.
A run that ended with a non-zero status is not repeated.  There is no tolerance in this file."""
import subprocess

import numpy as np
import pytest

import ssg_model as sm

pytestmark = pytest.mark.gpu

CASES = [c.name for c in sm.cases()] + ["g2_10000"]
RUNS = [(c, s) for c in CASES for s in sm.schedules_of(c)]
_DONE = {}


def tool(root, d, *ops):
    exe = root / "pathtracercuda_amd" / "lib" / "ssg_stages"
    assert exe.exists(), f"{exe} missing: run make"
    run = subprocess.run([str(exe), str(d), *ops], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, f"ssg_stages {' '.join(ops)}: exit status {run.returncode}: {run.stderr.strip()} {run.stdout.strip()}"


def once(key, make):
    """make() once per key; a failure is kept and raised again, the run is not repeated."""
    if key not in _DONE:
        try:
            _DONE[key] = (make(), None)
        except Exception as e:          # kept, to be raised again for every user of the run
            _DONE[key] = (None, e)
    val, err = _DONE[key]
    if err is not None:
        raise err
    return val


def words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else a.dtype)


def same(got, want, what):
    got, want = words(got), words(want)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert not len(bad), f"{what}: {len(bad)} of {want.size} words differ; first at {bad[0].tolist()}: device " \
                         f"{int(got[tuple(bad[0])]):#x}, model {int(want[tuple(bad[0])]):#x}"


def same_start(got, want, what):
    """Start records; an idle second phase is its first word alone (the kernel leaves the other seven as they were)."""
    idle = (want[:, :1, :] == sm.IDLE) & (np.arange(sm.START_WORDS)[None, :, None] > 0)
    same(np.where(idle, 0, got), np.where(idle, 0, want), what)


# ---- guess ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,spp,chunks", sm.GRID_CASES, ids=sm.GRID_IDS)
def test_guess_grid_equals_the_model(root, tmp_path, G, spp, chunks):
    cs, px, lim = sm.grid_case(G, spp, chunks)
    want = sm.guess(cs, px, px.pairs, lim)
    sm.write_case(tmp_path, cs, px)
    tool(root, tmp_path, "guess", "dump:g")
    same_start(sm.read_out(tmp_path, cs, "g")[0], want, "start records")


# ---- fold on the model's logs ------------------------------------------------------------------------
def fold_run(root, tmp, name, sched):
    def make():
        cs, px, tr, lim = sm.inputs(name)
        rounds, _ = sm.run(name, sched)              # the model first: its bounds assertions fire here
        d = tmp.mktemp("fold")
        start, L, _, _ = rounds[0]
        sm.write_case(d, cs, px, start=start, logs=L, state=sm.fold_state(cs, px), look=sm.SCHEDULES[sched][1])
        ops = ["fold:0", "dump:0"]
        for r in range(1, len(rounds)):
            ops += ["patch", f"fold:{r}", f"dump:{r}"]
        tool(root, d, *ops, "guess", "dump:g")
        return d
    return once(("fold", name, sched), make)


@pytest.mark.parametrize("name,sched", RUNS)
def test_fold_on_model_logs_equals_the_fold_model(root, tmp_path_factory, name, sched):
    cs, px, tr, lim = sm.inputs(name)
    d = fold_run(root, tmp_path_factory, name, sched)
    rounds, _ = sm.run(name, sched)
    for r, (start, L, P, S) in enumerate(rounds):
        _, _, gotP, got = sm.read_out(d, cs, str(r))
        assert got.dead == S.dead, f"round {r}: {got.dead} dead ends, model {S.dead}"
        same(got.accum, S.accum, f"round {r}: accum")
        same(got.rng, S.rng, f"round {r}: rng")
        same(got.fold, S.fold, f"round {r}: fold words")
        same(got.pairs, S.pairs, f"round {r}: pairs")
        if P is not None:
            same(gotP.count, P.count, f"round {r}: patch counts")
            live = np.arange(cs.cap)[None, :, None] < P.count[:, None, :]
            same(np.where(live, gotP.end, 0), np.where(live, P.end, 0), f"round {r}: patch end offsets")
            same(np.where(live[:, :, None, :], words(gotP.log), 0), np.where(live[:, :, None, :], words(P.log), 0), f"round {r}: patch log")
    # the next launch's guess from the statistics this fold wrote, at the states it left
    S = rounds[-1][3]
    at = np.where(S.fold[sm.F_FLAG] & 1, S.fold[sm.F_OFF], tr.off[cs.total]).astype(np.uint32)
    same_start(sm.read_out(d, cs, "g")[0], sm.guess(cs, px, S.pairs, lim, at=at), "start records after the fold")


# ---- lanes and chain on the device's own schedule ------------------------------------------------------
def chain_run(root, tmp, name):
    def make():
        cs, px, tr, lim = sm.inputs(name)
        sm.run(name, "earliest")                   # the model first
        d = tmp.mktemp("chain")
        sm.write_case(d, cs, px)
        tool(root, d, f"chain:{sm.ROUNDS}")
        return d
    return once(("chain", name), make)


def rounds_written(d):
    r = 0
    while (d / f"dead.{r + 1}.out").exists():
        r += 1
    return r


def getbit(bits, item, w, lane):
    return bool((int(bits[item, w // 64, lane]) >> (w % 64)) & 1)


def check_logs(cs, px, lim, start, L, F=None):
    """The logs of a lane launch against the stream and the rules; F: the fold words a patch round started from."""
    bad = []
    patch = F is not None
    J, G, cap, win64 = (1 if patch else cs.J), cs.G, cs.cap, cs.win * 64
    ks = np.arange(cap)[:, None]
    for pos in range(cs.tiles):
        v = lim[pos] >= 0
        li = np.where(v, lim[pos], 0)
        for j in range(J):
            it, g = pos * J + j, (G if patch else (j + 1) >> 1)
            if patch:
                active = v & ((F[sm.F_FLAG, li] & 1) == 1)
                base = F[sm.F_OFF, li]
                limit = np.minimum(cap, cs.total - F[sm.F_DONE, li])
                h0 = np.minimum(F[sm.F_H, li], G)
            else:
                base = np.zeros(64, np.uint32) if j == 0 else start[it, 0]
                active = v & (base != sm.IDLE)
                limit = np.full(64, cap)
                h0 = np.full(64, g + 1)
            base = np.where(active, base, 0).astype(np.uint32)
            cnt = L.count[it]
            if (cnt[~active] != 0).any() or (cnt[active] < 1).any() or (cnt > limit).any():
                bad.append(f"item {it}: counts {cnt.tolist()}")
                continue
            ends = L.end[it].astype(np.uint32)
            starts = base[None, :] + np.concatenate([np.zeros((1, 64), np.uint32), ends[:-1]])
            live = (ks < cnt[None, :]) & active[None, :]
            ln = sm.toy_len(px.tseed[li][None, :], px.cls[li][None, :], px.s0[li][None, :], px.s1[li][None, :], starts)
            col = sm.toy_colour(np.broadcast_to(px.tseed[li][None, :], starts.shape), starts)
            if (live & (base[None, :] + ends != starts + ln)).any():
                k, l = np.argwhere(live & (base[None, :] + ends != starts + ln))[0]
                bad.append(f"item {it} lane {l} sample {k}: ends at {int(base[l] + ends[k, l])}, the stream's sample from "
                           f"{int(starts[k, l])} takes {int(ln[k, l])}")
            got = words(L.log[it]).transpose(0, 2, 1)
            if (live[:, :, None] & (got != words(col))).any():
                bad.append(f"item {it}: a logged colour is not the stream's")
            if not patch:
                exp = np.zeros((cs.win, 64), np.uint64)
                if 1 <= g < G:
                    exp[0, active] |= np.uint64(1)
                    k, l = np.nonzero(live & (ends < win64))
                    np.bitwise_or.at(exp, (ends[k, l] // 64, l), np.uint64(1) << (ends[k, l] % 64).astype(np.uint64))
                if not np.array_equal(exp, L.bits[it]):
                    bad.append(f"item {it}: window bits are not the logged starts")
            for lane in np.flatnonzero(active):
                c = int(cnt[lane])
                rel = int(ends[c - 1, lane])
                off = int(base[lane]) + rel
                ok = c == int(limit[lane])
                if not patch and g + 1 == G and g >= 1:
                    ok = ok or off >= int(start[it, 7, lane])
                if not patch and j >= 2 and not (j & 1):
                    ok = ok or (rel + 1 < win64 and getbit(L.bits, it - 1, rel + 1, lane))
                    for Lk in cs.look:
                        if Lk and c > Lk:
                            wb = int(ends[c - 1 - Lk, lane]) + 1
                            ok = ok or (wb < win64 and getbit(L.bits, it - 1, wb, lane))
                h = int(h0[lane])
                so = lambda hh: int(start[pos * cs.J + 2 * hh - 1, 0, lane])
                while h < G and off > so(h) + win64:
                    h += 1
                while h + 1 < G and off >= so(h + 1):
                    h += 1
                if h < G and off >= so(h):
                    w, itA = off - so(h), pos * cs.J + 2 * h - 1
                    ok = ok or (w < win64 and getbit(L.bits, itA, w, lane)) or (w >= 1 and getbit(L.bits, itA + 1, w - 1, lane))
                if not ok:
                    bad.append(f"item {it} lane {lane}: stopped after {c} samples at offset {off} for no reason the rules allow")
    return bad


@pytest.mark.parametrize("name", CASES)
def test_lanes_log_the_stream_and_stop_by_the_rules(root, tmp_path_factory, name):
    cs, px, tr, lim = sm.inputs(name)
    d = chain_run(root, tmp_path_factory, name)
    start, L, _, _ = sm.read_out(d, cs, "0")
    same_start(start, sm.guess(cs, px, px.pairs, lim), "start records")
    bad = check_logs(cs, px, lim, start, L)
    for r in range(1, rounds_written(d) + 1):
        F = sm.read_out(d, cs, str(r - 1))[3].fold
        bad += [f"patch round {r}: {b}" for b in check_logs(cs, px, lim, start, sm.read_out(d, cs, str(r))[2], F=F)]
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("name", CASES)
def test_chain_equals_the_serial_truth(root, tmp_path_factory, name):
    cs, px, tr, lim = sm.inputs(name)
    d = chain_run(root, tmp_path_factory, name)
    bad, dead = [], []
    for r in range(rounds_written(d) + 1):
        S = sm.read_out(d, cs, str(r))[3]
        bad += sm.check_against_truth(cs, tr, lim, S, f"round {r}")
        flagged = int((S.fold[sm.F_FLAG][lim[lim >= 0]] & 1).sum())
        assert S.dead == flagged, f"round {r}: dead count {S.dead}, {flagged} pixels flagged"
        dead.append(S.dead)
    print(f"{name}: dead ends per round {dead}")
    assert not bad, "\n".join(bad[:12])
    assert dead[-1] == 0 or len(dead) == sm.ROUNDS + 1


# ---- the tool refuses what no lane can have written --------------------------------------------------
@pytest.mark.parametrize("what", ["count beyond cap", "entry beyond the tile grid", "records out of order", "bytes, the header asks for"])
def test_inconsistent_files_are_refused_before_any_launch(root, tmp_path, what):
    cs, px, _, _ = sm.inputs("g3_64")
    start, L, _, _ = sm.run("g3_64", "earliest")[0][0]
    sm.write_case(tmp_path, cs, px, start=start, logs=L, state=sm.fold_state(cs, px))
    if what == "count beyond cap":
        c = L.count.copy()
        c[3, 5] = cs.cap + 1
        c.tofile(tmp_path / "count.in")
    elif what == "entry beyond the tile grid":
        np.asarray([0x00010001, 0, 0x00020000, 1], np.uint32).tofile(tmp_path / "order.in")
    elif what == "records out of order":
        s = start.copy()
        s[3, 0, :] = s[1, 0, :]
        s.tofile(tmp_path / "start.in")
    else:
        L.end[:, :-1].tofile(tmp_path / "end.in")
    exe = root / "pathtracercuda_amd" / "lib" / "ssg_stages"
    run = subprocess.run([str(exe), str(tmp_path), "fold:0", "dump:0"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 1 and what in run.stderr, f"exit status {run.returncode}: {run.stderr.strip()}"
    assert not (tmp_path / "accum.0.out").exists()
