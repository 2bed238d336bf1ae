"""CPU models of the CTC forced alignment (wenet_amd/csrc/ctc_align.hip).

`ctc_align`      the plain rule, numpy, vectorised over the states: the
                 checker of the GPU tests.
`brute_force`    the best path by enumeration of all label-per-frame sequences (tiny cases).
`wave_form`      the one-wave kernel restated lane by lane: lane l owns NS consecutive states in
                 "registers", takes its left neighbour's last two values by a shuffle, keeps one
                 byte of back pointers per lane and frame, computes the states >= S like the
                 others, and walks the bytes backwards.
`block_form`     the general kernel: alphas of two frames in "LDS", four states (one byte of back
                 pointers) per thread step, only the reachable band worked on (states outside
                 keep whatever the buffers hold), back pointers of frame 0 never written.
`kernel_form`    dispatch like ctc_align_viterbi: wave form while S <= 256.
All return (path [T] int64, score float) or None when infeasible (status 1).
"""
import itertools

import numpy as np

FAST_S = 256


def feasible(T, y):
    return T >= len(y) + sum(y[i] == y[i - 1] for i in range(1, len(y)))


def ctc_align(logp, y, blank=0, dt=np.float32):
    """logp (T, V), y list of L ids -> (path [T], score) or None if infeasible."""
    T, L = logp.shape[0], len(y)
    lab = np.full(2 * L + 1, blank, np.int64); lab[1::2] = y
    S = lab.size
    if T < L + sum(y[i] == y[i - 1] for i in range(1, L)):
        return None
    E = logp[:, lab].astype(dt)                       # the emission gather
    skip = np.zeros(S, bool); skip[3::2] = lab[3::2] != lab[1:-2:2]
    ninf = dt(-np.inf)
    a = np.full(S, ninf, dt); a[:2] = E[0, :2]
    bp = np.zeros((T, S), np.int8)
    for t in range(1, T):
        x1 = np.concatenate(([ninf], a))[:S]
        x2 = np.where(skip, np.concatenate(([ninf, ninf], a))[:S], ninf)
        best, k = a.copy(), np.zeros(S, np.int8)
        m = x1 > best; best[m] = x1[m]; k[m] = 1
        m = x2 > best; best[m] = x2[m]; k[m] = 2
        a = (best + E[t]).astype(dt); bp[t] = k
    s = S - 1 if (S == 1 or a[S - 1] > a[S - 2]) else S - 2
    score, path = float(a[s]), np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = lab[s]; s -= int(bp[t, s])
    return path, score


def collapse(path, blank=0):
    out, prev = [], None
    for p in path:
        if p != prev and p != blank:
            out.append(int(p))
        prev = p
    return out


def brute_force(logp, y, blank=0):
    """Best score over every frame labelling that collapses to y (fp64) and all paths within
    1e-9 of it, or None."""
    T, V = logp.shape
    best, paths = -np.inf, []
    for path in itertools.product(range(V), repeat=T):
        if collapse(path, blank) != list(y):
            continue
        sc = float(sum(np.float64(logp[t, path[t]]) for t in range(T)))
        if sc > best + 1e-9:
            best, paths = sc, [path]
        elif abs(sc - best) <= 1e-9:
            paths.append(path)
    return (best, paths) if paths else None


def _emissions(logp, y, blank):
    """E (T, L + 1): column 0 blank, column 1 + i label i -- the gather kernel's output."""
    lab = np.asarray([blank] + list(y), np.int64)
    return logp[:, lab].astype(np.float32), lab


def wave_form(logp, y, blank=0, NS=None):
    T, L = logp.shape[0], len(y)
    S = 2 * L + 1
    if NS is None:
        NS = 1 if S <= 64 else 2 if S <= 128 else 4
    assert S <= 64 * NS
    if not feasible(T, y) or T == 0:
        return None
    E, lab = _emissions(logp, y, blank)
    f32, NINF = np.float32, np.float32(-np.inf)
    col = [[0] * NS for _ in range(64)]
    skip = [[False] * NS for _ in range(64)]
    al = [[NINF] * NS for _ in range(64)]
    for lane in range(64):
        for j in range(NS):
            s = lane * NS + j
            c = min((s + 1) >> 1, L) if s & 1 else 0
            col[lane][j] = c
            skip[lane][j] = bool((s & 1) and s >= 3 and s < S and lab[c] != lab[c - 1])
            al[lane][j] = E[0, 0] if s == 0 else E[0, 1] if (s == 1 and L > 0) else NINF
    bp = np.zeros((T, 64), np.uint8)
    for t in range(1, T):
        # the shuffles read the registers of frame t - 1 of every lane at once
        up1 = [al[lane - 1][NS - 1] if lane >= 1 else NINF for lane in range(64)]
        if NS >= 2:
            up2 = [al[lane - 1][NS - 2] if lane >= 1 else NINF for lane in range(64)]
        else:
            up2 = [al[lane - 2][0] if lane >= 2 else NINF for lane in range(64)]
        nxt = [[NINF] * NS for _ in range(64)]
        for lane in range(64):
            bits = 0
            for j in range(NS):
                x1 = al[lane][j - 1] if j >= 1 else up1[lane]
                x2c = al[lane][j - 2] if j >= 2 else (up1[lane] if j == 1 else up2[lane])
                x2 = x2c if skip[lane][j] else NINF
                best, k = al[lane][j], 0
                if x1 > best:
                    best, k = x1, 1
                if x2 > best:
                    best, k = x2, 2
                nxt[lane][j] = f32(best + E[t, col[lane][j]])
                bits |= k << (2 * j)
            bp[t, lane] = bits
        al = nxt
    v1 = al[(S - 1) // NS][(S - 1) % NS]
    v2 = al[(S - 2) // NS][(S - 2) % NS] if S >= 2 else NINF
    s = S - 1 if (S == 1 or v1 > v2) else S - 2
    score = float(v1 if s == S - 1 else v2)
    path = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = lab[(s + 1) >> 1] if s & 1 else blank
        s -= (int(bp[t, s // NS]) >> (2 * (s % NS))) & 3
    return path, score


def block_form(logp, y, blank=0, nthreads=256, junk=None):
    """`junk`: a random generator filling what the kernel leaves unwritten (back pointers
    outside the band and of frame 0), to show that nothing reads it."""
    T, L = logp.shape[0], len(y)
    S = 2 * L + 1
    if not feasible(T, y) or T == 0:
        return None
    E, lab = _emissions(logp, y, blank)
    f32, NINF = np.float32, np.float32(-np.inf)
    S16 = (S + 15) & ~15
    rowb = S16 >> 2
    bufs = [np.full(S16, NINF, f32), np.full(S16, NINF, f32)]
    bufs[0][0] = E[0, 0]
    if L > 0:
        bufs[0][1] = E[0, 1]
    if junk is None:
        bp = np.zeros((T, rowb), np.uint8)
    else:
        bp = junk.integers(0, 256, (T, rowb)).astype(np.uint8)
    p = 0
    for t in range(1, T):
        prev, cur = bufs[p], bufs[1 - p]
        lo = max(0, S - 2 * (T - t)) & ~3
        hi = min(S - 1, 2 * t + 1)
        g = lo >> 2
        while 4 * g <= hi:                 # (the threads' strided loop: groups are independent)
            s0 = 4 * g
            pv = [prev[s0 - 2] if s0 >= 2 else NINF, prev[s0 - 1] if s0 >= 1 else NINF] + \
                 [prev[s0 + j] for j in range(4)]
            bits = 0
            for j in range(4):
                s = s0 + j
                odd = j & 1
                c = min((s + 1) >> 1, L) if odd else 0
                sk = bool(odd and s >= 3 and s < S and lab[c] != lab[c - 1])
                e = E[t, c]
                x1, x2 = pv[1 + j], (pv[j] if sk else NINF)
                best, k = pv[2 + j], 0
                if x1 > best:
                    best, k = x1, 1
                if x2 > best:
                    best, k = x2, 2
                cur[s] = f32(best + e)
                bits |= k << (2 * j)
            bp[t, g] = bits
            g += 1
        p = 1 - p
    last = bufs[p]
    v1 = last[S - 1]
    v2 = last[S - 2] if S >= 2 else NINF
    s = S - 1 if (S == 1 or v1 > v2) else S - 2
    score = float(v1 if s == S - 1 else v2)
    path = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = lab[(s + 1) >> 1] if s & 1 else blank
        if t > 0:
            s -= (int(bp[t, s >> 2]) >> (2 * (s & 3))) & 3
    return path, score


def kernel_form(logp, y, blank=0):
    return wave_form(logp, y, blank) if 2 * len(y) + 1 <= FAST_S else block_form(logp, y, blank)


def random_case(rng, T, L, V, repeats=0.3, blank=0):
    """Random log-softmax rows and a label list of length L with adjacent repeats."""
    x = rng.standard_normal((T, V)).astype(np.float32) * 2.0
    x = x - np.log(np.exp(x.astype(np.float64)).sum(-1, keepdims=True)).astype(np.float32)
    ids = [v for v in range(V) if v != blank]
    y = []
    for i in range(L):
        if y and rng.random() < repeats:
            y.append(y[-1])
        else:
            y.append(int(rng.choice(ids)))
    return x, y


def repeats_of(y):
    return sum(y[i] == y[i - 1] for i in range(1, len(y)))
