"""NumPy float64 restatement of the streaming STFT and iSTFT (C ABI misonet_stft_stream /
misonet_istft_stream): the count formulas, the tail states, the existence rules and flush -- and, behind ``fault=``, the mistakes
a streaming front end is most likely to make, which tests/test_stream.py shows the exact-equality check rejects.

A frame is computed by one function of its 256 samples (``np.fft.rfft`` of one row), a hop by one function of the up to four
frames that exist, summed with t ascending: the streamed and the one-shot result are the same floating-point expressions, so they
are compared for exact equality, as the device tests compare the kernels."""
import numpy as np

HOP, NSEG, F = 64, 256, 129
TAIL, CARRY = 255, 3
MAX_N, MAX_T = 1 << 28, 1 << 22
WIN = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NSEG) / NSEG)          # periodic hann-256
WIN2 = WIN * WIN

FAULTS = ("tail_stuck", "tail_254", "tail_254_shifted", "phase_n_new", "missing_as_zero", "flush_full_envelope", "carry_2")


# ---- counts ----------------------------------------------------------------------------------------------------------------
def emitted_frames(N):
    """e(N): frame t is complete once sample 64 t + 127 has arrived"""
    return max(0, N // HOP - 1)


def emitted_hops(Tc):
    """g(Tc): hop h needs the frames h - 1 .. h + 2"""
    return max(0, Tc - 2)


def _ok(seen, new, flush, cap):
    return seen >= 0 and 0 <= new <= cap and (new >= 1 or bool(flush))


def stft_frames(n_seen, n_new, flush):
    if not _ok(n_seen, n_new, flush, MAX_N):
        return -1
    E = (n_seen + n_new) // HOP + 1 if flush else emitted_frames(n_seen + n_new)
    return E - emitted_frames(n_seen)


def istft_hops(t_seen, t_new, flush):
    if not _ok(t_seen, t_new, flush, MAX_T):
        return -1
    G = max(0, t_seen + t_new - 1) if flush else emitted_hops(t_seen + t_new)
    return G - emitted_hops(t_seen)


def pieces(total, cuts):
    """[(a, b)] covering [0, total): the cuts in turn (cycled), the last piece whatever is left"""
    out, a, i = [], 0, 0
    while a < total:
        b = min(total, a + cuts[i % len(cuts)])
        out.append((a, b))
        a, i = b, i + 1
    return out


# ---- analysis --------------------------------------------------------------------------------------------------------------
def _frame(seg):
    """seg float64 [..., 256] -> complex128 [..., 129]: X[f] = sum_j seg[j] hann[j] e^{-2 pi i f j / 256}, row by row"""
    return np.fft.rfft(seg * WIN, axis=-1)


def stft(x):
    """One shot: x float64 [L, M], L >= 1 -> complex128 [M, T, 129], T = L // 64 + 1; x = 0 outside [0, L)"""
    x = np.asarray(x, np.float64)
    L, M = x.shape
    T = L // HOP + 1
    p = np.zeros((128 + HOP * T + 128, M))
    p[128:128 + L] = x
    out = np.empty((M, T, F), np.complex128)
    for t in range(T):
        out[:, t] = _frame(p[HOP * t:HOP * t + NSEG].T)
    return out


class StftStream:
    """state: per microphone the last 255 samples, aligned to the stream's end, zero where it has not begun"""

    def __init__(self, M, fault=None):
        assert fault is None or fault in FAULTS
        self.M, self.fault = M, fault
        self.reset()

    def reset(self):
        self.tail = np.zeros((TAIL, self.M))
        self.n_seen, self.spent = 0, False

    def process(self, block, flush=False):
        """block float64 [n, M] -> complex128 [M, Tn, 129]"""
        assert not self.spent
        block = np.asarray(block, np.float64).reshape(-1, self.M)
        n, N = block.shape[0], self.n_seen
        Tn = stft_frames(N, n, flush)
        assert Tn >= 0
        # the virtual stream tail ++ block ++ zeros; sample p of it is sample N + p - 255 of the recording
        v = np.concatenate([self.tail, block, np.zeros((NSEG + HOP, self.M))])
        off0 = HOP * emitted_frames(N) - 128 - N                     # frame e(N) starts here, counted from the block's start:
        if self.fault == "phase_n_new":                              # -192 - N mod 64 once N >= 128
            off0 += N % HOP - n % HOP
        out = np.empty((self.M, Tn, F), np.complex128)
        for i in range(Tn):
            a = off0 + HOP * i + TAIL                                # ... and here in v
            seg = np.zeros((NSEG, self.M))
            lo = max(a, 0)
            if lo < a + NSEG:
                seg[lo - a:] = v[lo:a + NSEG]
            out[:, i] = _frame(seg.T)
        # "tail_254": the oldest sample is lost.  It is the sample a frame starts with 255 back, and hann[0] == 0 multiplies it:
        # no output can show this one.  "tail_254_shifted": the 254 kept samples sit one slot early, so every read is one off.
        keep = TAIL - 1 if self.fault in ("tail_254", "tail_254_shifted") else TAIL
        if self.fault != "tail_stuck":
            new = np.concatenate([self.tail, block])[-keep:]
            pad = np.zeros((TAIL - keep, self.M))
            self.tail = np.concatenate([new, pad] if self.fault == "tail_254_shifted" else [pad, new])
        self.n_seen, self.spent = N + n, bool(flush)
        return out


def stft_stream(x, cuts, fault=None, flush_with_block=True):
    """x [L, M] cut into pieces (``pieces``); the last piece goes in with flush, or before a flush that carries no block"""
    x = np.asarray(x, np.float64)
    st = StftStream(x.shape[1], fault)
    pc = pieces(x.shape[0], cuts)
    out = []
    for i, (a, b) in enumerate(pc):
        out.append(st.process(x[a:b], flush=flush_with_block and i == len(pc) - 1))
    if not flush_with_block:
        out.append(st.process(x[:0], flush=True))
    return np.concatenate(out, axis=1)


# ---- synthesis -------------------------------------------------------------------------------------------------------------
def _segment(X):
    """X complex128 [..., 129] -> float64 [..., 256]: w[k] irfft_256(X)[k]"""
    return np.fft.irfft(X, NSEG, axis=-1) * WIN


def _hop(z, exists, fault=None, is_flush_hop=False):
    """z: the windowed segments of the frames h - 1 .. h + 2 (None where the frame does not exist), t ascending -> the 64
    samples of hop h: sum w z / sum w^2 over the frames that exist"""
    sm, env = 0.0, np.zeros(HOP)
    for q in range(4):
        k = slice(192 - HOP * q, 256 - HOP * q)
        if exists[q]:
            sm = sm + z[q][..., k]
            env = env + WIN2[k]
        elif fault == "missing_as_zero":
            env = env + WIN2[k]                                      # added as zero WITH its envelope term
    if fault == "flush_full_envelope" and is_flush_hop:
        env = np.full(HOP, 1.5)
    return sm / env


def istft(X):
    """One shot: X complex128 [R, T, 129], T >= 2 -> float64 [R, 64 (T - 1)]"""
    X = np.asarray(X, np.complex128)
    R, T, _ = X.shape
    z = _segment(X)
    out = np.empty((R, HOP * (T - 1)))
    for h in range(T - 1):
        ex = [0 <= h - 1 + q < T for q in range(4)]
        out[:, HOP * h:HOP * (h + 1)] = _hop([z[:, h - 1 + q] if ex[q] else None for q in range(4)], ex)
    return out


class IstftStream:
    """state: per row the last 3 frames"""

    def __init__(self, R, fault=None):
        assert fault is None or fault in FAULTS
        self.R, self.fault = R, fault
        self.reset()

    def reset(self):
        self.carry = np.zeros((self.R, CARRY, F), np.complex128)
        self.t_seen, self.spent = 0, False

    def process(self, X, flush=False):
        """X complex128 [R, Tn, 129] -> float64 [R, 64 H]"""
        assert not self.spent
        X = np.asarray(X, np.complex128).reshape(self.R, -1, F)
        Tn, Tc = X.shape[1], self.t_seen
        H = istft_hops(Tc, Tn, flush)
        assert H >= 0
        v = np.concatenate([self.carry, X], axis=1)                  # frame t of the stream is v[:, t - Tc + 3]
        z = _segment(v)
        g0, Tend = emitted_hops(Tc), Tc + Tn
        out = np.empty((self.R, HOP * H))
        for i in range(H):
            h = g0 + i
            ex = [0 <= h - 1 + q < Tend for q in range(4)]
            zs = [z[:, h - 1 + q - Tc + CARRY] if ex[q] else None for q in range(4)]
            out[:, HOP * i:HOP * (i + 1)] = _hop(zs, ex, self.fault, flush and h == Tend - 2)
        keep = 2 if self.fault == "carry_2" else CARRY
        self.carry = np.concatenate([np.zeros((self.R, CARRY - keep, F), np.complex128), v[:, v.shape[1] - keep:]], axis=1)
        self.t_seen, self.spent = Tend, bool(flush)
        return out


def istft_stream(X, cuts, fault=None, flush_with_block=True):
    X = np.asarray(X, np.complex128)
    st = IstftStream(X.shape[0], fault)
    pc = pieces(X.shape[1], cuts)
    out = []
    for i, (a, b) in enumerate(pc):
        out.append(st.process(X[:, a:b], flush=flush_with_block and i == len(pc) - 1))
    if not flush_with_block:
        out.append(st.process(X[:, :0], flush=True))
    return np.concatenate(out, axis=1)


def to_int16(y):
    """(short)(int)(y * 32767.0f) of the float32 value"""
    return (np.asarray(y, np.float32) * np.float32(32767.0)).astype(np.int32).astype(np.int16)
