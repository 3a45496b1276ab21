"""The cases that hold the stacked-Gram bin solver (csrc/stacked_gram.hpp: wpe_bin_k of wpe.hip, wpd_bin_k of wpd.hip) to float64 at
every order and tile edge, and the tile arithmetic they are chosen by, in one place.  Pure Python: no device, no library.

The solver stages T through LDS 64 frames at a time and builds the 2K x 2K real Gram matrix of [Re s; Im s] (K = M (taps + 1)) in
16 x 16 tiles, lower half, dealt round-robin to 8 waves: every branch of it depends on M, taps, T or delay.  ``geometry`` restates
that arithmetic (sg_tiles_init, sg_zpitch); tests/test_sg_cases.py asserts on the CPU that the lists below, with the shapes the
older device tests run, reach every such branch, that their inputs are well conditioned and that the bars reject every planted
fault; tests/test_gpu_sg_edges.py runs them on the device.

A case is (B, M, T, F, taps, delay), the tuple of the older tests.
"""
TILE = 64            # SG_TT: frames per LDS tile
WAVES = 8            # SG_WAVES
SLOTS = 9            # SG_SLOTS: accumulator tiles per wave
MFMA = 16            # rows of an MFMA tile
WPE_NMAX = 80        # misonet_wpe: 1 <= M <= 8, M taps <= 80
WPD_KMAX = 88        # misonet_wpd: 2 <= M <= 8, M (taps + 1) <= 88
OUT_BAR = 2.4e-7     # 4 x 2^-24: one complex64 rounding of a float64 result (the bar of test_gpu_wpe.py and test_gpu_wpd.py)


def geometry(M, taps):
    """the integers the scheme branches on: K = M (taps + 1), 2K, NT = ceil(2K / 16) tile rows, ntiles = NT (NT + 1) / 2, the
    accumulator slots of wave 0 .. 7 (tile tau goes to wave tau % 8) and zl = 64 + taps - 1, the frames of a staged z window"""
    K = M * (taps + 1)
    NT = -(-2 * K // MFMA)
    ntiles = NT * (NT + 1) // 2
    slots = tuple(max(0, -(-(ntiles - wave) // WAVES)) for wave in range(WAVES))
    return dict(K=K, K2=2 * K, NT=NT, ntiles=ntiles, slots=slots, zl=TILE + taps - 1)


def admitted(kernel):
    """every (M, taps) the host check of the kernel admits"""
    if kernel == "wpe":
        return [(M, taps) for M in range(1, 9) for taps in range(1, WPE_NMAX // M + 1)]
    return [(M, taps) for M in range(2, 9) for taps in range(1, WPD_KMAX // M)]


def _order_T(order):
    return max(130, 2 * order + 70)


# ---- every order: (M, taps) with delay = 3, T = max(130, 2 order + 70) (order = M taps for WPE, K for WPD), F = 2 ------------------
# NT 1, 1, 2, 2, 3, 4, 4, 4, 5, 6, 7, 8, 9, 10, 11, 11, 11 and 1, 1, 2, 2, 3, 4, 4, 4, 5, 6, 7, 8, 9, 10, 11, 11; 2K = 0 (mod 16)
# at (8, 3), (8, 7), (8, 9) and 2 (mod 16) at (3, 2), (5, 4), (1, 80); (5, 3) is there for NT = 3, which nothing else reaches.
# The long filters of WPE need more frames than that rule gives before the restatement itself is insensitive enough
# (test_sg_cases.py, the conditioning tests, which also have the figures at the T that were refused).
ORDERS_WPE_MT = [(1, 1), (1, 7), (3, 2), (5, 2), (5, 3), (5, 4), (7, 3), (8, 3), (7, 4), (5, 8), (7, 7), (8, 7), (7, 9), (8, 9),
                 (7, 11), (2, 40), (1, 80)]
ORDERS_WPD_MT = [(2, 1), (2, 3), (3, 2), (5, 2), (5, 3), (5, 4), (7, 3), (8, 3), (7, 4), (5, 8), (7, 7), (8, 7), (7, 9), (8, 9),
                 (7, 11), (2, 43)]
LONG_T = {(2, 40): 300, (1, 80): 2000}
ORDERS_WPE = [(1, M, LONG_T.get((M, taps), _order_T(M * taps)), 2, taps, 3) for M, taps in ORDERS_WPE_MT]
ORDERS_WPD = [(1, M, _order_T(M * (taps + 1)), 2, taps, 3) for M, taps in ORDERS_WPD_MT]

# ---- T at the edges of one and of two tiles, for both kernels: the last tile exactly full, one frame short, one frame long ----------
T_EDGES = [(1, M, T, 3, taps, delay) for M, taps, delay in [(2, 2, 1), (3, 3, 2)] for T in (63, 64, 65, 127, 128, 129)]

# ---- delay around and past one tile, for both kernels: the history of a tile lies wholly outside the tile before it -----------------
DELAY_EDGES = [(1, 2, 200, 3, 3, delay) for delay in (62, 63, 64, 65, 70, 130)]

# ---- WPE only: delay >= T, so Z = 0, R = 0 and the bin is passed through (WPD refuses T <= delay + taps - 1 on the host).  Not
# delay = T - 1 or another almost-empty Z: there the rank is deficient and the flag depends on rounding ---------------------------------
WPE_PASS_THROUGH = [(1, 2, T, 3, taps, delay) for T, delay, taps in [(2, 3, 1), (5, 5, 1), (70, 70, 2)]]

# ---- the shapes the older device tests run (test_gpu_wpe.py SHAPES and its full size; wpd_ref.SHAPES), restated for the coverage -----
OLD_WPE = [(2, 4, 60, 9, 3, 2), (1, 2, 40, 5, 2, 1), (1, 6, 300, 17, 10, 3), (1, 8, 200, 3, 10, 3), (1, 3, 12, 4, 3, 1),
           (1, 6, 1001, 129, 10, 3)]
OLD_WPD = [(2, 4, 60, 9, 3, 2), (1, 2, 40, 5, 2, 1), (1, 3, 70, 4, 3, 1), (1, 6, 300, 17, 5, 3), (1, 8, 200, 3, 10, 3)]

# ---- WPE with power_floor = 0.05, a floor that binds, on a second tile of one frame (WPD has wpd_ref.SHAPES[2] for it) -----------------
FLOOR = 0.05
FLOOR_WPE = (1, 3, 65, 3, 3, 2)

NEW_WPE = ORDERS_WPE + T_EDGES + DELAY_EDGES
NEW_WPD = ORDERS_WPD + T_EDGES + DELAY_EDGES


def case_id(case):
    return "x".join(map(str, case))


def per_frame(a, b, axes):
    """the worst rel-L2 of one frame: norms over ``axes`` of a - b and of b, the largest quotient (numpy arrays)"""
    import numpy as np
    a, b = np.asarray(a), np.asarray(b)
    num = np.sqrt(np.sum(np.abs(a - b) ** 2, axis=axes))
    den = np.sqrt(np.sum(np.abs(b) ** 2, axis=axes))
    return float(np.max(num / den))
