"""The weight-gradient planner on the CPU: spp-rl_amd/csrc/dw_plan.h's plan_dw (split assignment, slab arena, item
table: what finalize_dw uploads for the kernels of csrc/dw.hip), printed by tests/dw_plan_dump.cpp, a stand-alone g++
program built with the address and undefined-behaviour sanitizers and run as a child process, over
  job lists   the agents' phases as build_dw composes them (SAC fp32 and bf16, DDPG, and the ACM / BasicAcM regression
              sets) at every AGENT_DIMS, and the lists of the direct GPU test (tests/dw_cases.py)
  Bp          32 .. 819,200, around the LDS kernels' threshold (8,160 / 8,192 / 8,224 / 8,256) and its 64-sample rule
  num_cu      1, 3, 64, 256, 304
and checked for the invariants the kernels rely on.  The step counts and kinds that the GPU cases' parametrisation
states (dw_cases.LDS32, LDS64, edge_wanted) are checked here too, against the same function."""
import os
import shutil
import subprocess

import pytest

import dw_cases as dc
from test_cpu_layout import AGENT_DIMS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BPS = [32, 64, 96, 2048, 8160, 8192, 8224, 8256, 65536, 409600, 819200]
CUS = [1, 3, 64, 256, 304]


def cdiv(a, b):
    return -(-a // b)


def fused_nsplit(Bp, cu):
    """Slabs of a fused fc3 job: one per wave of the phase kernel's grid (4 waves per workgroup, at most one
    workgroup per CU)."""
    return 4 * max(1, min(cdiv(Bp // 32, 4), cu))


def agent_sets():
    """{name: [phase 0 jobs, phase 1 jobs]}, a job = (N, K0, K1, bf16, a_bf, x_bf, fused), as build_dw lists them."""
    out = {}
    for ob, aout, ac, acmc in AGENT_DIMS:
        ca = ac if acmc else aout
        tag = "%d_%d_%d_%d" % (ob, aout, ac, acmc)
        for bf in (0, 1):
            critic = [(256, ob, ca, bf, bf, 0, 0), (256, 256, 0, bf, bf, bf, 0),
                      (1, 256, 0, bf, 0, bf, 0) if bf else (1, 256, 0, 0, 0, 0, 1)]  # bf16 sets: fc3 is a k_dw job
            actor = [(256, ob, 0, bf, bf, 0, 0), (256, 256, 0, bf, bf, bf, 0), (2 * aout, 256, 0, bf, 0, bf, 0)]
            out["sac%s_%s" % ("_bf16" if bf else "", tag)] = [2 * critic, actor]
            out["acm%s_%s" % ("_bf16" if bf else "", tag)] = [[(64, 2 * ob, 0, bf, 0, 0, 0), (32, 64, 0, bf, 0, 0, 0),
                                                               (ac, 32, 0, bf, 0, 0, 0)]]
        out["ddpg_" + tag] = [[(256, ob, ca, 0, 0, 0, 0), (256, 256, 0, 0, 0, 0, 0), (1, 256, 0, 0, 0, 0, int(ob <= 32))],
                              [(256, ob, 0, 0, 0, 0, 0), (256, 256, 0, 0, 0, 0, 0), (aout, 256, 0, 0, 0, 0, 0)]]
        out["bacm_" + tag] = [[(100, 2 * ob, 0, 0, 0, 0, 0), (50, 100, 0, 0, 0, 0, 0), (50, 2 * ob, 0, 0, 0, 0, 0),
                               (ac, 50, 0, 0, 0, 0, 0)]]
    return out


def direct_sets():
    """The direct GPU test's lists: every shape alone (fp32 and all-bf16 rows) and the whole phases."""
    out = {}
    for i, (N, K0, K1, _) in enumerate(dc.SHAPES):
        for mode in ("fp32", "bf16_bb"):
            out["shape%d_%s" % (i, mode)] = [[(N, K0, K1) + dc.MODES[mode] + (0,)]]
    for name, make in dc.PHASES.items():
        for bf in (0, 1):
            out["phase_%s_%d" % (name, bf)] = [[(N, K0, K1, bf, a, x, f) for N, K0, K1, _, a, x, f in make(bf)]]
    return out


def single(N, K0, K1, mode):
    return [[(N, K0, K1) + dc.MODES[mode] + (0,)]]


def queries():
    """[(name, phases, Bp, num_cu, fused nsplit)] in the order the program answers them."""
    q = []
    for name, phases in list(agent_sets().items()) + list(direct_sets().items()):
        for Bp in BPS:
            for cu in CUS:
                q.append((name, phases, Bp, cu, fused_nsplit(Bp, cu)))
    for B, cu, *_ in dc.LDS32:
        q.append(("lds32", single(256, 256, 0, "fp32"), dc.rup(B, 32), cu, 0))
    for B, cu, *_ in dc.LDS64:
        q.append(("lds64", single(256, 256, 0, "bf16_bb"), dc.rup(B, 32), cu, 0))
    q.append(("fallback", single(256, 256, 0, "bf16_bb"), 8224, 29, 0))
    for B in dc.EDGE_BATCHES:
        for i, (N, K0, K1, _) in enumerate(dc.EDGE_SHAPES):
            for cu in dc.EDGE_CUS:
                q.append(("edge_%d_%d" % (B, i), single(N, K0, K1, "fp32"), dc.rup(B, 32), cu, 0))
    for name, make in dc.PHASES.items():
        for B, cu in dc.PHASE_RUNS:
            for bf in (0, 1):
                q.append(("phaserun_%s_%d" % (name, bf), [[(N, K0, K1, bf, a, x, f) for N, K0, K1, _, a, x, f in make(bf)]],
                          dc.rup(B, 32), cu, dc.PHASE_FUSED_NSPLIT))
    return q


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """[(query, plan)] with plan = {"need", "jobs": [dict], "phases": [{"nitems", "nlds", "max_elems", "items"}]}"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    tmp = tmp_path_factory.mktemp("dw_plan")
    exe = str(tmp / "dw_plan_dump")
    # (the sanitizer runtimes are linked into the program: nothing about them depends on the environment it runs in)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           os.path.join(REPO, "tests", "dw_plan_dump.cpp"), "-o", exe])
    qs = queries()
    lines, last = [], None
    for name, phases, Bp, cu, fns in qs:
        if (name, phases) != last:
            lines.append("set " + name)
            for p, jobs in enumerate(phases):
                if p:
                    lines.append("phase")
                lines += ["job %d %d %d %d %d %d %d" % j for j in jobs]
            last = (name, phases)
        lines.append("run %d %d %d" % (Bp, cu, fns))
    src = tmp / "queries.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
    out, cur = [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "plan":
            cur = {"name": w[1], "Bp": int(w[2]), "cu": int(w[3]), "need": int(w[5]), "jobs": [], "phases": []}
            out.append(cur)
        elif w[0] == "job":
            keys = ("idx", "phase", "N", "K0", "K1", "bf16", "a_bf", "x_bf", "fused")
            j = dict(zip(keys, map(int, w[1:10])))
            j.update({w[k]: int(w[k + 1]) for k in range(10, len(w), 2)})
            cur["jobs"].append(j)
        elif w[0] == "phase":
            cur["phases"].append({"nitems": int(w[3]), "nlds": int(w[5]), "max_elems": int(w[7])})
        else:
            assert w[0] == "items"
            runs = list(map(int, w[2:]))
            cur["phases"][int(w[1])]["items"] = [(runs[k], runs[k + 1] + t) for k in range(0, len(runs), 3)
                                                 for t in range(runs[k + 2])]
    assert len(out) == len(qs)
    for (name, _, Bp, cu, _), p in zip(qs, out):
        assert (p["name"], p["Bp"], p["cu"]) == (name, Bp, cu)
    return list(zip(qs, out))


def is_big(j):
    return dc.rup(j["N"], 32) * dc.rup(j["K0"] + j["K1"], 32) >= 128 * 128


def is_lds(j, Bp):
    return (Bp >= 8192 and j["N"] == 256 and j["K0"] == 256 and j["K1"] == 0 and
            (not j["bf16"] or (j["a_bf"] and j["x_bf"] and Bp % 64 == 0)))


def test_splits_are_whole_units_and_cover_the_batch(plans):
    n = 0
    for (name, _, Bp, cu, fns), p in plans:
        for j in p["jobs"]:
            if j["fused"]:
                assert (j["nsplit"], j["wsplit"]) == (fns, 1)
                continue
            tn, tk = j["N"] <= 128, j["K0"] + j["K1"] <= 128
            assert j["wsplit"] == (4 if tn and tk else 2 if tn != tk else 1), (name, j)
            unit = 64 if is_lds(j, Bp) and j["bf16"] else 32 * j["wsplit"]
            assert j["split_len"] > 0 and j["split_len"] % unit == 0, (name, Bp, cu, j)
            assert j["nsplit"] == cdiv(Bp, j["split_len"]) >= 1, (name, Bp, cu, j)
            assert (j["nsplit"] - 1) * j["split_len"] < Bp, (name, Bp, cu, j)  # the last split holds samples
            n += 1
    assert n > 10000


def test_item_table_lists_every_split_once_large_jobs_first(plans):
    for (name, phases, Bp, cu, _), p in plans:
        assert len(p["phases"]) == len(phases)
        for ph, P in enumerate(p["phases"]):
            jobs = [j for j in p["jobs"] if j["phase"] == ph]
            want = sorted((k, s) for k, j in enumerate(jobs) if not j["fused"] for s in range(j["nsplit"]))
            assert sorted(P["items"]) == want and P["nitems"] == len(want), (name, Bp, cu, ph)
            cls = [0 if is_lds(jobs[k], Bp) else 1 if is_big(jobs[k]) else 2 for k, _ in P["items"]]
            assert cls == sorted(cls), (name, Bp, cu, ph)
            assert P["nlds"] == cls.count(0), (name, Bp, cu, ph)


def test_slab_regions_are_disjoint_and_inside_the_arena(plans):
    for (name, phases, Bp, cu, _), p in plans:
        for ph in range(len(phases)):
            regions = []
            for j in p["jobs"]:
                if j["phase"] != ph:
                    continue
                nslab = j["nsplit"] * j["wsplit"]
                el = j["N"] * (j["K0"] + j["K1"]) + j["N"]
                assert j["slab_stride"] >= el and j["slab_stride"] % 4 == 0
                if nslab == 1:
                    assert j["slab_off"] == -1, (name, Bp, cu, j)  # stored directly
                    continue
                assert j["slab_off"] >= 0 and j["slab_off"] % 4 == 0, (name, Bp, cu, j)
                regions.append((j["slab_off"], j["slab_off"] + nslab * j["slab_stride"]))
            regions.sort()
            for (a0, a1), (b0, b1) in zip(regions, regions[1:]):
                assert a1 <= b0, (name, Bp, cu, ph)
            assert not regions or regions[-1][1] <= p["need"], (name, Bp, cu, ph)


def test_reduce_grid_covers_every_job(plans):
    for (name, _, Bp, cu, _), p in plans:
        for j in p["jobs"]:
            el = j["N"] * (j["K0"] + j["K1"]) + j["N"]
            group = 16 if j["nsplit"] * j["wsplit"] >= 64 and el <= 4096 else 1  # dw_red_group
            assert p["phases"][j["phase"]]["max_elems"] >= el * group, (name, Bp, cu, j)


def _plan(p, k=0):
    j = p["jobs"][k]
    return (j["split_len"], j["nsplit"], j["wsplit"])


def test_gpu_cases_state_the_plans_they_run(plans):
    """The step counts written in the direct GPU test's parametrisation, and the kinds its batch-edge cases reach."""
    by = {}
    for (name, _, Bp, cu, _), p in plans:
        by.setdefault(name, {})[(Bp, cu)] = p
    for tab, name, step in ((dc.LDS32, "lds32", 32), (dc.LDS64, "lds64", 64)):
        for B, cu, steps, last, items in tab:
            Bp = dc.rup(B, 32)
            p = by[name][(Bp, cu)]
            assert p["phases"][0]["nlds"] == items, (name, B, cu)
            assert _plan(p) == (step * steps, items, 1) and Bp - (items - 1) * step * steps == step * last, (name, B, cu)
        assert {1, 2, 3} <= {t[2] for t in tab} and any(8 <= t[2] <= 10 for t in tab), name
        assert any(t[2] >= 43 for t in tab) and any(t[3] < t[2] for t in tab), name
    p = by["fallback"][(8224, 29)]
    assert p["phases"][0]["nlds"] == 0 and _plan(p) == (288, 29, 1)
    for B in dc.EDGE_BATCHES:
        Bp, seen = dc.rup(B, 32), set()
        for i in range(len(dc.EDGE_SHAPES)):
            for cu in dc.EDGE_CUS:
                seen |= dc.edge_kinds(_plan(by["edge_%d_%d" % (B, i)][(Bp, cu)]), Bp)
        assert dc.edge_wanted(Bp) <= seen, (B, dc.edge_wanted(Bp) - seen)
    # the whole phases: at Bp >= 8192 LDS items, other large items and thin items share the table (bf16 at Bp = 8224:
    # no LDS item); at B = 100 no LDS item
    for name in dc.PHASES:
        for B, cu in dc.PHASE_RUNS:
            for bf in (0, 1):
                Bp = dc.rup(B, 32)
                p = by["phaserun_%s_%d" % (name, bf)][(Bp, cu)]
                nlds = p["phases"][0]["nlds"]
                assert (nlds > 0) == (Bp >= 8192 and (not bf or Bp % 64 == 0)), (name, B, bf)
                assert p["phases"][0]["nitems"] > nlds


def test_shape_list_reaches_every_tile_instantiation():
    """The coverage accounting of the direct GPU test's shape list (pure arithmetic, from k_dw's rule): all 16 fp32
    tile shapes under wsplit 4, 2 and 1, each with and without the bias sum, and the 9 bf16 shapes under every wsplit."""
    for db in (True, False):
        got = set().union(*(dc.tiles_of(N, K0 + K1, db, 0) for N, K0, K1, _ in dc.SHAPES))
        for ws in (4, 2, 1):
            assert {(i, j) for w, i, j, _ in got if w == ws} == dc.ALL16, ws
        assert {(i, j, b) for _, i, j, b in got} >= {(i, j, db) for i, j in dc.ALL16}
    got = set().union(*(dc.tiles_of(N, K0 + K1, True, 1) for N, K0, K1, _ in dc.SHAPES))
    for ws in (4, 2, 1):
        assert {(i, j) for w, i, j, _ in got if w == ws} == dc.ALL9, ws
    assert any(K1 and K0 % 32 for _, K0, K1, _ in dc.SHAPES) and any(K1 == 0 for _, _, K1, _ in dc.SHAPES)
    assert any(n2 and n2 % 32 for *_, n2 in dc.SHAPES) and any(n2 and n2 % 32 == 0 for *_, n2 in dc.SHAPES)
    used = {s for N, K0, K1, _ in dc.SHAPES for s in (N, K0 + K1)}
    assert {1, 22, 33, 64, 65, 96, 100, 128, 129, 160, 222, 225, 256, 14, 23, 119} <= used
