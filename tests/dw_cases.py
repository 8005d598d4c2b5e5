"""The job lists of the direct weight-gradient tests (tests/test_gpu_dw_direct.py), shared with the planner's CPU
test (tests/test_cpu_dw_plan.py, which checks on the CPU the plans and step counts the GPU cases are written for),
and the coverage accounting of k_dw's tile instantiations.  Data and pure arithmetic only: no GPU, no library."""


def rup(x, m):
    return (x + m - 1) // m * m


# (N, K0, K1, nrow2): sides from {1, 22, 33, 64, 65, 96, 100, 128, 129, 160, 192, 222, 225, 256} (1 .. 8 blocks of 32,
# each block count above 4 with its remainder 1 .. 4 beside a full quadrant); K1 > 0 with K0 no multiple of 32
# (14 = 11 + 3, 23 = 17 + 6, 119 = 111 + 8, 222 = 111 + 111, ...); nrow2 inside a block and at a block edge
SHAPES = [
    # wsplit 4: N, K <= 128, the 16 (blocks of N, blocks of K)
    (1, 1, 0, None), (22, 64, 0, 11), (1, 65, 0, None), (22, 100, 0, None),
    (33, 11, 3, None), (64, 33, 0, 32), (33, 96, 0, None), (64, 111, 8, None),
    (65, 17, 6, None), (96, 64, 0, 64), (65, 65, 0, None), (96, 128, 0, None),
    (100, 22, 0, None), (128, 33, 0, None), (100, 90, 6, 50), (128, 128, 0, 96),
    # wsplit 2, N <= 128 < K: ni = blocks of N, nj = 4 and blocks of K - 4
    (1, 129, 0, None), (22, 192, 0, 11), (22, 111, 111, None), (1, 256, 0, None),
    (33, 160, 0, None), (64, 100, 92, None), (64, 222, 0, None), (33, 225, 0, None),
    (65, 129, 0, None), (96, 192, 0, None), (65, 222, 0, None), (96, 129, 0, 95),
    (100, 160, 0, None), (100, 192, 0, None), (128, 222, 0, 64),
    # wsplit 2, K <= 128 < N: nj = blocks of K, ni = 4 and blocks of N - 4
    (129, 22, 0, None), (192, 1, 0, None), (222, 22, 0, 111), (256, 11, 0, None),
    (160, 33, 0, 128), (192, 64, 0, None), (222, 33, 0, None),
    (129, 65, 0, None), (192, 96, 0, None), (222, 90, 6, None), (256, 11, 3, None),
    (160, 100, 0, None), (192, 128, 0, 96), (222, 111, 8, 111), (256, 128, 0, None),
    # wsplit 1: (blocks of N - 4, blocks of K - 4), with the three full-quadrant shapes beside each
    (129, 129, 0, None), (160, 192, 0, 128), (129, 111, 111, None),
    (192, 160, 0, None), (192, 100, 92, 191), (192, 222, 0, None),
    (222, 129, 0, 111), (222, 192, 0, None), (222, 111, 111, 111),
    (225, 256, 0, None), (256, 225, 0, 129), (256, 256, 0, None),
]
# name: (bf16, a_bf, x_bf)
MODES = {"fp32": (0, 0, 0), "bf16_ff": (1, 0, 0), "bf16_bf": (1, 1, 0), "bf16_bb": (1, 1, 1), "bf16_fb": (1, 0, 1)}
ALL16 = {(i, j) for i in range(1, 5) for j in range(1, 5)}
ALL9 = {(i, j) for i in (1, 2, 4) for j in (1, 2, 4)}

# the batch-edge cases' shapes, each alone in its phase at EDGE_CUS
EDGE_SHAPES = [(256, 256, 0, None), (222, 111, 111, 111), (100, 222, 0, None), (222, 100, 0, None), (100, 128, 0, 50),
               (22, 11, 3, 11), (129, 160, 0, None)]
EDGE_BATCHES = [1, 31, 32, 33, 97, 130, 1001]
EDGE_CUS = [1, 3, 64]

# One 256 x 256 job on the LDS-DMA kernels: (B, num_cu, steps of a full item, steps of the last item, items), worked
# out from plan_dw: ns = min(num_cu, Bp / 32); split_len = round_up(cdiv(Bp, ns), step); nsplit = cdiv(Bp, split_len).
# fp32 (k_dw_big, k_dw_big8): a step is 32 samples
LDS32 = [(8192, 256, 1, 1, 256), (8193, 256, 2, 1, 129), (8192, 128, 2, 2, 128), (8192, 86, 3, 1, 86),
         (8193, 86, 3, 2, 86), (8192, 29, 9, 4, 29), (8193, 29, 9, 5, 29), (8192, 3, 86, 84, 3), (8193, 3, 86, 85, 3),
         (8192, 1, 256, 256, 1)]
# bf16 A and X rows, Bp % 64 == 0 (k_dw_big16): a step is 64 samples
LDS64 = [(8192, 128, 1, 1, 128), (8192, 64, 2, 2, 64), (8192, 43, 3, 2, 43), (8192, 3, 43, 42, 3), (8230, 129, 1, 1, 129),
         (8230, 14, 10, 9, 13), (8230, 3, 43, 43, 3), (8192, 1, 128, 128, 1)]


# whole phases: (N, K0, K1, nrow2, a_bf, x_bf, fused) with the bf16 sets' element types where bf is set
def critic_phase(bf):
    """Two critics x [fc1 256 x (11 + 3), fc2 256 x 256, fused fc3 1 x 256]"""
    return 2 * [(256, 11, 3, None, bf, 0, 0), (256, 256, 0, None, bf, bf, 0), (1, 256, 0, None, 0, 0, 1)]


def actor_phase(bf):
    """[fc1 256 x 11, fc2 256 x 256, head 22 x 256 with nrow2 = 11]"""
    return [(256, 11, 0, None, bf, 0, 0), (256, 256, 0, None, bf, bf, 0), (22, 256, 0, 11, 0, bf, 0)]


PHASES = {"critic": critic_phase, "actor": actor_phase}
PHASE_RUNS = [(100, 256), (8192, 256), (8200, 64)]  # (B, num_cu); 8200: Bp = 8224, no multiple of 64
PHASE_FUSED_NSPLIT = 1024


def tiles_of(N, K, db, bf16):
    """{(wsplit, NI, NJ, bias sum)} that k_dw's four waves instantiate for an N x K job (dw.hip: k_dw): wsplit from
    N, K <= 128, the wave's quadrant (nb0, kb0), ni, nj; the bf16 forms run a 3-block side as 4."""
    tn, tk = N <= 128, K <= 128
    ws = 4 if tn and tk else (2 if tn != tk else 1)
    out = set()
    for w in range(4):
        nb0, kb0 = 4 * (w >> 1), 4 * (w & 1)
        if ws == 4:
            nb0 = kb0 = 0
        elif ws == 2:
            if tn:
                nb0 = 0
            else:
                kb0 = 0
        ni = min(4, max(0, (N + 31) // 32 - nb0))
        nj = min(4, max(0, (K + 31) // 32 - kb0))
        if ni == 0 or nj == 0:
            continue
        if bf16:
            ni, nj = (4 if ni == 3 else ni), (4 if nj == 3 else nj)
        out.add((ws, ni, nj, bool(db and kb0 == 0)))
    return out


def unit_stats(plan, Bp):
    """Of a planned job (split_len, nsplit, wsplit): (32-sample units of a full item's wave part, units of each wave
    part of the last item), by k_dw's partition of an item into wsplit parts of whole units."""
    split_len, nsplit, ws = plan
    last = Bp - (nsplit - 1) * split_len
    q = rup(-(-last // ws), 32)
    parts = [max(0, min(q, last - p * q)) // 32 for p in range(ws)]
    return split_len // ws // 32, parts


def edge_kinds(plan, Bp):
    """What a batch-edge case exercises, from its plan."""
    full, parts = unit_stats(plan, Bp)
    out = {"one slab" if plan[1] * plan[2] == 1 else "several slabs", "1 unit" if full == 1 else "several units"}
    if plan[1] > 1 and sum(parts) * 32 < plan[0]:
        out.add("ragged last item")
    if plan[2] > 1 and 0 in parts:
        out.add("empty wave part")
    return out


# what the shapes x EDGE_CUS of one batch size must reach between them (checked on the CPU against plan_dw)
def edge_wanted(Bp):
    want = {"one slab", "several slabs", "1 unit"}
    if Bp >= 128:
        want.add("several units")
    if Bp == 1024:
        want.add("ragged last item")
    if Bp <= 64 or Bp == 160:
        want.add("empty wave part")
    return want
