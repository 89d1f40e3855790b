"""The launch policy and the build table on the CPU.

pathtracercuda_amd/csrc/pt_launch_plan.h decides what a render launches from plain values, and
pt_builds.h holds one row per trace-kernel build; tools/launch_plan_check.cpp (built with ASan/UBSan by
the Makefile) prints both.  Checked here:

  * the automatic build and its LDS bytes against the hand-written policy of tests/size_scenes.py, for
    the scenes tests/test_gpu_size_scenes.py part C launches, at 256 compute units (where the build is
    also the literal in the table) and at 64 and 304;
  * the build table against size_scenes.BUILDS, and the LDS function against size_scenes.LDS_CASES;
  * the exclusions between launch modes, which the GPU suite sees only through bit-exact results.
"""
import json
import pathlib
import subprocess

import pytest

import bvh_edit as be
import size_scenes as ss

ROOT = pathlib.Path(__file__).resolve().parents[1]
EXE = ROOT / "pathtracercuda_amd" / "lib" / "launch_plan_check"
CUS = (256, 64, 304)
CHILD_BOX_BUILDS = (20, 39, 40, 41, 46, 47, 48, 60, 61, 91)


def ask(lines):
    """One JSON object per request line; a sanitizer report or a request the program rejects fails."""
    run = subprocess.run([str(EXE)], input="".join(line + "\n" for line in lines), capture_output=True, text=True,
                         timeout=60)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-2000:]
    return [json.loads(line) for line in run.stdout.splitlines()]


def plan(**inputs):
    return ask(["plan " + " ".join(f"{k}={int(v)}" for k, v in inputs.items())])[0]


def scene_args(name):
    I, R, nodes, prims = ss.SIZES[name]
    sc = ss.case(name)
    # (a scene outside the child-box encoding has no records: pt_set_scene uploads none)
    return dict(nodes=nodes, records=I if sc.child_box_ok else 0, prims=prims, rows=R, hasRecords=sc.child_box_ok,
                dfsOrder=be.dfs_ordered(sc.nodes))


# ---- the automatic build ------------------------------------------------------------------------
@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("frame,table", [(ss.large_frame, ss.AUTO_LARGE), (ss.small_frame, ss.AUTO_SMALL)],
                         ids=["large", "small"])
def test_automatic_build(frame, table, cus):
    W, H = frame(cus)
    tx, ty = (W + 7) // 8, (H + 7) // 8
    if frame is ss.large_frame:
        assert tx * ty >= 4 * cus * 24
    else:
        assert tx * ty <= 16 * cus
    names = list(table)
    # a first launch of 2 spp x 2 calls, every knob at its default (test_automatic_build_* on the GPU)
    got = ask(["plan " + " ".join(f"{k}={int(v)}" for k, v in dict(cus=cus, tilesX=tx, tilesY=ty, spp=2, chunks=2,
                                                                      **scene_args(n)).items()) for n in names])
    assert len(got) == len(names)
    for name, p in zip(names, got):
        I, R, nodes, prims = ss.SIZES[name]
        a = scene_args(name)
        build, lds = ss.expected_build(I, R, nodes, prims, a["hasRecords"], a["dfsOrder"], tx * ty, tx * ty, cus)
        if cus == 256:
            assert build == table[name], f"{name}: the table disagrees with the written expectation"
        assert p["refusal"] is None and p["K"] == 1 and p["G"] == 0 and p["units"] == tx * ty, (name, p)
        assert (p["build"], p["lds"]) == (build, lds), (name, cus, p, "the documented policy", build, lds)


# ---- the table and the LDS function -------------------------------------------------------------
def test_build_table_agrees_with_size_scenes():
    rows = {r["id"]: r for r in ask(["builds"])}
    assert sorted(rows) == [1, 4, 6, 20, 39, 40, 41, 46, 47, 48, 60, 61, 90, 91]
    for build, (staged, wpb, child_box) in ss.BUILDS.items():
        r = rows[build]
        assert (r["SL"], r["WPB"], bool(r["childBox"])) == (staged, wpb, child_box), (build, r)
    assert [b for b, r in rows.items() if not r["settable"]] == [90]
    # modes: bit m = uninstrumented MODE m, bit 6 = the instrumented kernel
    assert {b: r["modes"] for b, r in rows.items()} == {
        1: 0x41, 20: 0x41, 47: 0x41, 48: 0x41, 4: 0x61, 6: 0x61, 39: 0x47, 40: 0x7f, 41: 0x7f, 46: 0x7f, 60: 0x7f, 61: 0x7f,
        90: 0x01, 91: 0x01}


def test_lds_function_on_the_staging_limits():
    reqs = []
    for name, build, _, _ in ss.LDS_CASES:
        I, R, nodes, prims = ss.SIZES[name]
        reqs.append(f"lds build={build} nodes={nodes} records={I} prims={prims} rows={R}")
    got = ask(reqs)
    for (name, build, lds, staged), g in zip(ss.LDS_CASES, got):
        assert (g["bytes"], g["SL"]) == (lds, staged), (name, build, g)


# ---- exclusions between the modes ---------------------------------------------------------------
# the smallest inputs: one tile, a scene of one record; a launch of 16 samples is the shortest that
# gets a cold start, one of 4 lies in automatic run-ahead's range
FORCED = dict(stripMode=4, ssgMode=4, aheadMode=2)


@pytest.mark.parametrize("knobs", [{}, {"stripMode": 4}, {"ssgMode": 4}, {"aheadMode": 2}, FORCED,
                                   dict(FORCED, stashMatches=1, orderValid=1, orderStale=0, orderSamples=16)],
                         ids=["defaults", "strips", "groups", "run-ahead", "all", "all-warm"])
def test_instrumented_launch_is_plain(knobs):
    for spp, chunks in ((16, 1), (8, 2), (2, 2)):
        p = plan(instrumented=1, spp=spp, chunks=chunks, **knobs)
        assert p["refusal"] is None and p["mode"] == "instrumented", p
        assert (p["K"], p["G"], p["aheadUse"], p["aheadMake"], p["cold"]) == (1, 0, 0, 0, "none"), p


@pytest.mark.parametrize("build", (0, 40, 41, 46, 60, 61))
def test_forced_strips(build):
    for extra in ({}, {"ssgMode": 4}, {"stashMatches": 1}):
        p = plan(variant=build, stripMode=4, spp=2, chunks=2, **extra)
        assert (p["mode"], p["K"], p["G"], p["aheadUse"], p["aheadMake"]) == ("strip", 4, 0, 0, 0), p
    # (a stash-making knob outranks them, and a build without strip units runs plain)
    assert plan(variant=build, stripMode=4, aheadMode=2, spp=2, chunks=2)["K"] == 1
    assert plan(variant=47, stripMode=4, spp=2, chunks=2)["mode"] == "plain"


@pytest.mark.parametrize("build", (0, 39, 40, 41, 46, 60, 61))
def test_forced_groups(build):
    for extra in ({}, {"stashMatches": 1}):
        p = plan(variant=build, ssgMode=4, spp=4, chunks=2, **extra)
        assert (p["mode"], p["G"], p["K"], p["aheadUse"], p["aheadMake"]) == ("grouped", 4, 1, 0, 0), p
        assert p["ssgCap"] == 8 and p["mainPrio"][3] == 0, p
    assert plan(variant=build, ssgMode=4, spp=1, chunks=2)["G"] == 2          # at most one group per sample
    assert plan(variant=48, ssgMode=4, spp=4, chunks=2)["G"] == 0


@pytest.mark.parametrize("build", (0, 40, 41, 46, 60, 61))
def test_run_ahead_always(build):
    for extra in ({}, {"stripMode": 4}, {"ssgMode": 4}, FORCED, {"spp": 1, "chunks": 1}, {"spp": 64, "chunks": 64}):
        p = plan(**dict(dict(variant=build, aheadMode=2, spp=4, chunks=2), **extra))
        assert (p["mode"], p["K"], p["G"], p["aheadMake"]) == ("ahead", 1, 0, 1), p
    assert plan(variant=39, aheadMode=2, spp=4, chunks=2)["mode"] == "plain"


def test_rise_repair_off():
    for build in (40, 60, 0):                          # (a one-record scene's automatic build is 60)
        p = plan(variant=build, riseRepair=0, spp=2, chunks=2)
        assert (p["refusal"], p["build"], p["mode"], p["K"], p["G"], p["aheadMake"]) == (None, 90, "plain", 1, 0, 0), p
        p = plan(variant=build, riseRepair=0, spp=2, chunks=2, **FORCED)
        assert (p["build"], p["mode"]) == (90, "plain"), p
        assert "pt_set_rise_repair(0)" in plan(variant=build, riseRepair=0, instrumented=1)["refusal"]
    for build in (1, 4, 6, 20, 39, 41, 46, 47, 48, 61, 91):
        assert "pt_set_rise_repair(0)" in plan(variant=build, riseRepair=0)["refusal"], build
    # the automatic choice of a cache-read scene, and of one without records
    assert plan(riseRepair=0, records=769, nodes=1539, prims=770, rows=12)["refusal"]
    assert plan(riseRepair=0, records=0, hasRecords=0)["refusal"]


@pytest.mark.parametrize("build", CHILD_BOX_BUILDS)
@pytest.mark.parametrize("missing", [dict(hasRecords=0, records=0), dict(dfsOrder=0)], ids=["no-records", "no-dfs-order"])
def test_forced_child_box_build_without_its_layout(build, missing):
    for nodes, want in ((1536, 6), (1537, 4)):         # 32 B a node: 48 KB exactly, and the next
        p = plan(**dict(dict(variant=build, nodes=nodes, records=(nodes - 1) // 2, prims=nodes, rows=10, spp=2, chunks=2,
                             stripMode=4), **missing))
        assert (p["build"], p["mode"], p["K"], p["G"], p["aheadMake"]) == (want, "plain", 1, 0, 0), p
    for node_walk in (1, 4, 6):                        # the node-at-a-time builds stay as forced
        assert plan(**dict(dict(variant=node_walk, nodes=1537), **missing))["build"] == node_walk
