"""The weight-gradient kernels (csrc/dw.hip) on their own, against a plain reference of the same operation:
    dW = A[:, :B] @ concat(X0, X1)[:, :B].T,   db = A[:, :B].sum(1),   rows >= nrow2 in the second output,
through sppDebugDwSet: the agents' planner (plan_dw with a num_cu the test chooses), item table, slab arena, launch
function and kernels.

Exact cases (the bulk).  The operands are small integers, so every product and every partial sum, in any order, is
an integer below 2^24 and therefore exact in fp32: the kernels' result must EQUAL the reference, bit for bit.  Every
case asserts the condition (max over elements of sum_b |a| |x| < 2^24, and sum_b |a| < 2^24 for db) on the CPU before
it launches.  The reference is a float64 matrix product of the integer operands, exact below 2^53.  A dropped or
doubled sample, a wrong row, seam, slab or split is an integer difference with no tolerance to hide in.  The four
outputs of a job lie in one buffer between guard words, pre-filled with a sentinel: nothing outside the [N][K] and
[N] images may change, and the slab arena starts as NaN (sppDebugDwSet), so a slab word that is summed without having
been written shows too.

Dead columns B .. Bp - 1 (the kernels sum over all Bp): A is zero there, as the per-sample kernels guarantee for every
layer-output gradient; X holds non-zero integers, as a layer input may (spprl.h, sppDebugDwSet).

Rounding cases (bf16 jobs, fp32-element operands): integers that bf16 cannot hold -- odd values in +-[257, 511] (all
ties) and values in +-[513, 1023] (ties and both directions) -- against operands rounded by oracle.bf16.rne: dW
bit-equal separates round-to-nearest-even from truncation and from round-half-away.  db sums the A rows as stored:
the unrounded fp32 values for fp32 rows, the bf16 values for bf16 rows.  oracle/bf16.py's backward states the same
(Mode.db: HEAD sums the unrounded delta, HIDDEN the rounded one), so kernel and oracle agree and that is the reference.

Float cases (a few): Gaussian operands (bf16 jobs: pre-rounded with rne) against float64 with the derived bound
    |got - ref| <= (Bp + nslab) 2^-24 sum_b |a| |x|
(one rounding per multiply-add of a Bp-term sum in any order, plus the slab sums; products of bf16 values are exact in
fp32, so the bound serves both precisions).  They exist so that nothing depends on integer operands.

Coverage accounting (never used as an expected value): from the kernel's rule -- wsplit from N, K <= 128, the wave's
quadrant (nb0, kb0), ni, nj -- the tile-shape tests compute which (wsplit, NI, NJ) each case reaches and assert that
the list reaches all 16 fp32 shapes (with and without the bias sum) under wsplit 4, 2 and 1, and the 9 bf16 shapes
under every wsplit in each of the 4 operand-element modes.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

import dw_cases as dc  # noqa: E402
from dw_cases import MODES, rup  # noqa: E402
from oracle import bf16 as obf  # noqa: E402
from spprl import _lib  # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 63  # guard words around every output image
SENTINEL = -12345.625
LIMIT = 1 << 24


class Job:
    """One job and its operands.  A / X are int64 or float64 numpy arrays [rows][Bp] holding the values the
    kernel is given (already representable in the element type)."""

    def __init__(self, N, K0, K1=0, nrow2=None, db=True, bf16=0, a_bf=0, x_bf=0, fused=False, nsplit=0):
        self.N, self.K0, self.K1, self.K = N, K0, K1, K0 + K1
        self.nrow2 = N if nrow2 is None else nrow2
        self.db, self.bf16, self.a_bf, self.x_bf, self.fused, self.nsplit = db, bf16, a_bf, x_bf, fused, nsplit
        self.A = self.X = self.slabs = None

    def name(self):
        return "%dx(%d+%d) nrow2 %d db %d bf16 %d a_bf %d x_bf %d%s" % (
            self.N, self.K0, self.K1, self.nrow2, self.db, self.bf16, self.a_bf, self.x_bf,
            " fused x%d" % self.nsplit if self.fused else "")


def amax_for(Bp):
    """Largest integer magnitude with Bp a^2 < 2^24, at most 256 (exact in bf16), at least 4."""
    return max(4, min(256, math.isqrt((LIMIT - 1) // Bp)))


def fill_int(job, rng, B, amax=None):
    Bp = rup(B, 32)
    m = amax or amax_for(Bp)
    assert m <= 4 or Bp * m * m < LIMIT
    job.A = rng.randint(-m, m + 1, (job.N, Bp)).astype(np.int64)
    job.A[:, B:] = 0
    job.X = rng.randint(-m, m + 1, (job.K, Bp)).astype(np.int64)
    dead = job.X[:, B:]
    dead[dead == 0] = m  # non-zero in every dead column


def fill_slabs(job, rng):
    el = job.N * job.K + job.N
    stride = rup(el, 4)
    job.slabs = np.full((job.nsplit, stride), 3.0e7, np.float64)  # the padding words are never summed
    job.slabs[:, :el] = rng.randint(-1000, 1001, (job.nsplit, el))


def reference(job, B):
    """(dW [N][K], db [N], sum |a||x| [N][K], sum |a| [N]) in float64."""
    if job.fused:
        el = job.N * job.K + job.N
        s, a = job.slabs[:, :el].sum(0), np.abs(job.slabs[:, :el]).sum(0)
        return (s[:job.N * job.K].reshape(job.N, job.K), s[job.N * job.K:], a[:job.N * job.K].reshape(job.N, job.K),
                a[job.N * job.K:])
    A, X = job.A[:, :B].astype(np.float64), job.X[:, :B].astype(np.float64)
    return A @ X.T, A.sum(1), np.abs(A) @ np.abs(X).T, np.abs(A).sum(1)


def _dev(a, bf):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16 if bf else torch.float32)


def run(jobs, B, num_cu, big_waves=4):
    """Launch the jobs as one phase.  Returns [(dW [N][K], db [N] or None, plan)] with plan = (split_len, nsplit,
    wsplit); asserts that every guard word and every output the job does not own kept the sentinel."""
    Bp = rup(B, 32)
    descs = (_lib.DwJobDesc * len(jobs))()
    keep, outs = [], []
    for d, j in zip(descs, jobs):
        n2 = j.N - j.nrow2
        sizes = [j.nrow2 * j.K, j.nrow2 if j.db else 0, n2 * j.K, n2 if j.db else 0]
        offs, o = [], GUARD
        for s in sizes:
            offs.append(o)
            o += s + GUARD  # (no alignment: a net's tensors lie back to back in its gradient buffer)
        buf = torch.full((o,), SENTINEL, dtype=torch.float32, device=DEV)
        outs.append((buf, offs, sizes))
        p = buf.data_ptr()
        d.dW = p + 4 * offs[0]
        d.db = p + 4 * offs[1] if j.db else None
        d.dW2 = p + 4 * offs[2] if n2 else None
        d.db2 = p + 4 * offs[3] if n2 and j.db else None
        d.N, d.K0, d.K1, d.nrow2 = j.N, j.K0, j.K1, j.nrow2
        d.bf16, d.a_bf, d.x_bf, d.fused, d.nsplit = j.bf16, j.a_bf, j.x_bf, int(j.fused), j.nsplit
        if j.fused:
            t = _dev(j.slabs, False)
            keep.append(t)
            d.slabs = t.data_ptr()
        else:
            assert j.A.shape == (j.N, Bp) and j.X.shape == (j.K, Bp)
            a, x0 = _dev(j.A, j.a_bf), _dev(j.X[:j.K0], j.x_bf)
            keep += [a, x0]
            d.A, d.X0 = a.data_ptr(), x0.data_ptr()
            if j.K1:
                x1 = _dev(j.X[j.K0:], j.x_bf)
                keep.append(x1)
                d.X1 = x1.data_ptr()
    torch.cuda.synchronize()
    _lib.call("sppDebugDwSet", descs, len(jobs), B, num_cu, big_waves, _lib.stream_handle())
    torch.cuda.synchronize()
    res = []
    for d, j, (buf, offs, sizes) in zip(descs, jobs, outs):
        h = buf.cpu().numpy()
        own = np.zeros(h.shape, bool)
        for o, s in zip(offs, sizes):
            own[o:o + s] = True
        assert (h[~own] == np.float32(SENTINEL)).all(), "%s: %d words outside the job's images were written" % (
            j.name(), int((h[~own] != np.float32(SENTINEL)).sum()))
        dW = np.concatenate([h[offs[0]:offs[0] + sizes[0]], h[offs[2]:offs[2] + sizes[2]]]).reshape(j.N, j.K)
        db = np.concatenate([h[offs[1]:offs[1] + sizes[1]], h[offs[3]:offs[3] + sizes[3]]]) if j.db else None
        res.append((dW, db, (d.split_len, d.nsplit, d.wsplit)))
    return res


def check_exact(jobs, B, num_cu, big_waves=4, what=""):
    """The integer condition, then bit-equality of every job of the phase.  Returns the plans."""
    refs = [reference(j, B) for j in jobs]
    for j, (_, _, aw, ab) in zip(jobs, refs):
        assert aw.max() < LIMIT and ab.max() < LIMIT, "%s: the operands are too large for exact fp32 sums" % j.name()
    got = run(jobs, B, num_cu, big_waves)
    for j, (rw, rb, _, _), (dW, db, plan) in zip(jobs, refs, got):
        tag = "%s B %d num_cu %d waves %d %s plan %s" % (what, B, num_cu, big_waves, j.name(), plan)
        np.testing.assert_array_equal(dW.astype(np.float64), rw, err_msg="dW " + tag)
        if j.db:
            np.testing.assert_array_equal(db.astype(np.float64), rb, err_msg="db " + tag)
    return [g[2] for g in got]


# ------------------------------------------------------------------ every tile shape of k_dw
@pytest.mark.parametrize("db", [True, False], ids=["db", "nodb"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_tile_shape_exact(mode, db):
    """B = 97 (Bp = 128: four 32-sample units, the last with one live sample), num_cu = 2: items of one or two units.
    The accounting (dw_cases.tiles_of, k_dw's rule; never an expected value) asserts what the list reached."""
    bf, a_bf, x_bf = MODES[mode]
    reached = set()
    for i, (N, K0, K1, n2) in enumerate(dc.SHAPES):
        j = Job(N, K0, K1, n2, db, bf, a_bf, x_bf)
        fill_int(j, np.random.RandomState(1000 + i), 97)
        check_exact([j], 97, 2, what=mode)
        reached |= dc.tiles_of(N, K0 + K1, db, bf)
    for ws in (4, 2, 1):
        assert {(a, b) for w, a, b, _ in reached if w == ws} == (dc.ALL9 if bf else dc.ALL16), (mode, ws)
    assert {(a, b) for _, a, b, s in reached if s == db} == (dc.ALL9 if bf else dc.ALL16)
    print("coverage %s db=%d: %d (wsplit, NI, NJ, bias sum): %s" % (mode, db, len(reached), sorted(reached)))


# ------------------------------------------------------------------ batch edges
@pytest.mark.parametrize("B", dc.EDGE_BATCHES)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_batch_edges_exact(mode, B):
    """Each shape alone at num_cu 1, 3 and 64: one item (a > 128 x > 128 job then stores directly), ragged items of
    several units, one unit per item; the thin shapes' empty wave parts come with the small batches."""
    bf, a_bf, x_bf = MODES[mode]
    Bp = rup(B, 32)
    seen = set()
    for i, (N, K0, K1, n2) in enumerate(dc.EDGE_SHAPES):
        for cu in dc.EDGE_CUS:
            j = Job(N, K0, K1, n2, True, bf, a_bf, x_bf)
            fill_int(j, np.random.RandomState(B + 7 * i), B)
            (plan,) = check_exact([j], B, cu, what=mode)
            seen |= dc.edge_kinds(plan, Bp)
    assert dc.edge_wanted(Bp) <= seen, (dc.edge_wanted(Bp) - seen, B)


@pytest.mark.parametrize("mode", ["fp32", "bf16_bb"])
def test_direct_store_of_one_slab(mode):
    """nsplit * wsplit == 1: a > 128 x > 128 job at Bp = 32 stores to dW / dW2 / db / db2 without slabs."""
    bf, a_bf, x_bf = MODES[mode]
    j = Job(222, 111, 111, 111, True, bf, a_bf, x_bf)
    fill_int(j, np.random.RandomState(5), 32)
    (plan,) = check_exact([j], 32, 304, what=mode)
    assert plan[1] * plan[2] == 1


# ------------------------------------------------------------------ LDS-DMA kernels (step counts: dw_cases.LDS32 / LDS64)
@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("B,cu,steps,last,items", dc.LDS32)
def test_lds_fp32_exact(B, cu, steps, last, items, waves):
    """k_dw_big (4) and k_dw_big8 (8), each against the reference; items of `steps` 32-sample steps, the last of `last`."""
    Bp = rup(B, 32)
    j = Job(256, 256, 0, 128 if cu == 29 else None, db=cu != 86)
    fill_int(j, np.random.RandomState(B + cu), B)
    (plan,) = check_exact([j], B, cu, waves, what="lds")
    assert plan == (32 * steps, items, 1) and Bp - (items - 1) * 32 * steps == 32 * last


@pytest.mark.parametrize("B,cu,steps,last,items", dc.LDS64)
def test_lds_bf16_exact(B, cu, steps, last, items):
    """k_dw_big16: bf16 A and X rows, Bp % 64 == 0 (B = 8230: Bp = 8256), 64-sample steps."""
    Bp = rup(B, 32)
    assert Bp % 64 == 0
    j = Job(256, 256, 0, 128 if cu == 14 else None, db=cu != 43, bf16=1, a_bf=1, x_bf=1)
    fill_int(j, np.random.RandomState(B + cu), B)
    (plan,) = check_exact([j], B, cu, what="lds16")
    assert plan == (64 * steps, items, 1) and Bp - (items - 1) * 64 * steps == 64 * last


@pytest.mark.parametrize("mode", ["bf16_bb", "bf16_ff", "bf16_bf"])
def test_bf16_256_falls_back_to_register_tiles(mode):
    """B = 8193, Bp = 8224 (no multiple of 64), or an fp32 operand row: k_dw<true> in 32-sample units."""
    bf, a_bf, x_bf = MODES[mode]
    j = Job(256, 256, 0, None, True, bf, a_bf, x_bf)
    fill_int(j, np.random.RandomState(11), 8193)
    (plan,) = check_exact([j], 8193, 29, what=mode)
    assert plan == (288, 29, 1)  # cdiv(8224, 29) = 284 -> 288: 9 units, the last item 5


# ------------------------------------------------------------------ whole phases in one call
PHASE_CASES = [(ph, bf, w, B, cu) for ph in sorted(dc.PHASES) for bf in (0, 1) for w in ((4,) if bf else (4, 8))
               for B, cu in dc.PHASE_RUNS]  # (big_waves reaches the fp32 sets only: the bf16 sets have one LDS kernel)


@pytest.mark.parametrize("phase,bf,waves,B,cu", PHASE_CASES)
def test_whole_phase_exact(phase, bf, waves, B, cu):
    """LDS items, other large items, thin items and reduce-only jobs in one item table and one arena, distinct data
    per job; at B = 100 everything runs in k_dw.  (B = 8200: Bp = 8224, the bf16 256 x 256 jobs stay in k_dw.)"""
    rng = np.random.RandomState(B + cu + waves)
    jobs = [Job(N, K0, K1, n2, True, bf, a, x, bool(f), dc.PHASE_FUSED_NSPLIT if f else 0)
            for N, K0, K1, n2, a, x, f in dc.PHASES[phase](bf)]
    for j in jobs:
        fill_slabs(j, rng) if j.fused else fill_int(j, rng, B)
    plans = check_exact(jobs, B, cu, waves, what="phase")
    assert len(set(plans)) > 1


# ------------------------------------------------------------------ reduce
@pytest.mark.parametrize("nsplit", [2, 16, 63, 64, 100, 257, 1024])
def test_reduce_of_caller_filled_slabs(nsplit):
    """257-element images (a critic's fused fc3): one lane per element below 64 slabs, 16-lane groups from 64 on
    (dw_red_group), with a ragged last round of 16 x 16 slabs; with and without the bias element."""
    rng = np.random.RandomState(nsplit)
    jobs = [Job(1, 256, 0, None, True, fused=True, nsplit=nsplit), Job(1, 256, 0, None, False, fused=True, nsplit=nsplit),
            Job(2, 64, 64, 1, True, fused=True, nsplit=nsplit)]
    for j in jobs:
        fill_slabs(j, rng)
    check_exact(jobs, 64, 8, what="reduce")


def test_reduce_of_a_thin_job_with_many_slabs():
    """3 x 32 at Bp = 32768: 16 items x 4 wave parts = 64 slabs of 99 elements -> the 16-lane-group reduce."""
    j = Job(3, 32, 0, 2, True)
    fill_int(j, np.random.RandomState(3), 32768 - 5)
    (plan,) = check_exact([j], 32768 - 5, 256, what="thin")
    assert plan[1] * plan[2] >= 64 and 3 * 32 + 3 <= 4096


# ------------------------------------------------------------------ rounding (bf16 jobs, fp32-element operands)
def _unrepresentable(rng, shape, kind):
    if kind == "ties":  # odd values in +-[257, 511]: bf16 spacing 2 there, every one a tie
        v = 2 * rng.randint(128, 256, shape) + 1
    else:  # +-[513, 1023]: spacing 4; remainders 1 (down), 2 (tie), 3 (up)
        v = rng.randint(513, 1024, shape)
        v[v % 4 == 0] += 1
    return (v * rng.choice([-1, 1], shape)).astype(np.int64)


@pytest.mark.parametrize("kind,B", [("ties", 40), ("mixed", 12)])
@pytest.mark.parametrize("mode", ["bf16_ff", "bf16_bf", "bf16_fb"])
@pytest.mark.parametrize("N,K0,K1,n2", [(256, 256, 0, None), (22, 11, 3, 11), (100, 222, 0, None)])
def test_bf16_rounding_is_nearest_even(N, K0, K1, n2, mode, kind, B):
    """fp32 rows hold integers bf16 cannot represent; the reference rounds them with oracle.bf16.rne.  db sums the
    rows as stored (unrounded for fp32 rows).  Few live samples: 40 x 512^2 and 12 x 1024^2 stay below 2^24."""
    bf, a_bf, x_bf = MODES[mode]
    rng = np.random.RandomState(N + B)
    Bp = rup(B, 32)
    j = Job(N, K0, K1, n2, True, bf, a_bf, x_bf)
    fill_int(j, rng, B, amax=256)
    if not a_bf:
        j.A = _unrepresentable(rng, j.A.shape, kind)
        j.A[:, B:] = 0
    if not x_bf:
        j.X = _unrepresentable(rng, j.X.shape, kind)
    rnd = lambda a: obf.rne(torch.from_numpy(a.astype(np.float32))).double().numpy()  # noqa: E731
    Ar, Xr = rnd(j.A)[:, :B], rnd(j.X)[:, :B]
    if not a_bf:
        assert (Ar != j.A[:, :B]).all()
    if not x_bf:
        assert (Xr != j.X[:, :B]).all()
    assert (np.abs(Ar) @ np.abs(Xr).T).max() < LIMIT and np.abs(j.A).sum(1).max() < LIMIT
    ((dW, db, plan),) = run([j], B, 8)
    np.testing.assert_array_equal(dW.astype(np.float64), Ar @ Xr.T, err_msg="dW %s %s" % (j.name(), plan))
    np.testing.assert_array_equal(db.astype(np.float64), j.A[:, :B].astype(np.float64).sum(1), err_msg="db " + j.name())
    assert Bp % 32 == 0


# ------------------------------------------------------------------ float operands
FLOAT_SHAPES = [(256, 256, 0, None, 1001, 8, 4), (22, 11, 3, 11, 1001, 8, 4), (256, 256, 0, 128, 8193, 29, 4),
                (256, 256, 0, 128, 8230, 14, 4)]  # (.., B, num_cu, big_waves); 8230: Bp = 8256, k_dw_big16 for bf16_bb
FLOAT_CASES = [t + (m,) for t in FLOAT_SHAPES for m in ("fp32", "bf16_bb", "bf16_ff")] + [
    (256, 256, 0, None, 8193, 29, 8, "fp32")]


@pytest.mark.parametrize("N,K0,K1,n2,B,cu,waves,mode", FLOAT_CASES)
def test_gaussian_operands_within_the_derived_bound(N, K0, K1, n2, B, cu, waves, mode):
    bf, a_bf, x_bf = MODES[mode]
    rng = np.random.RandomState(B + N)
    Bp = rup(B, 32)
    j = Job(N, K0, K1, n2, True, bf, a_bf, x_bf)
    A, X = rng.randn(N, Bp).astype(np.float32), rng.randn(K0 + K1, Bp).astype(np.float32)
    A[:, B:] = 0
    if bf:  # pre-rounded: the conversion itself is the rounding cases' subject
        A, X = obf.rne(torch.from_numpy(A)).numpy(), obf.rne(torch.from_numpy(X)).numpy()
    j.A, j.X = A.astype(np.float64), X.astype(np.float64)
    rw, rb, aw, ab = reference(j, B)
    ((dW, db, plan),) = run([j], B, cu, waves)
    f = (Bp + plan[1] * plan[2]) * 2.0 ** -24
    ew, eb = np.abs(dW - rw) / (f * aw), np.abs(db - rb) / (f * ab)
    print("float case %s %s plan %s: dW err / bound %.3g, db err / bound %.3g" % (mode, j.name(), plan, ew.max(), eb.max()))
    assert ew.max() <= 1.0 and eb.max() <= 1.0
    assert np.abs(dW).max() > 1.0


def test_arguments_are_validated():
    d = (_lib.DwJobDesc * 1)()
    d[0].N, d[0].K0, d[0].nrow2 = 300, 4, 300
    lib = _lib.load()
    assert lib.sppDebugDwSet(d, 1, 32, 8, 4, None) != 0 and b"debug dw" in lib.sppGetLastError()
    assert lib.sppDebugDwSet(d, 1, 32, 8, 5, None) != 0
