"""Operator tests of the `attention` decode mode's kernels (csrc/attn_search.hip) through the hooks
wn_op_attn_self_step / wn_op_attn_step_embed / wn_op_attn_prompt_cache / wn_op_beam_init /
wn_op_beam_update / wn_op_beam_finish -- the launchers beam_search_run calls -- against the plain
references of tests/kernel_refs.py (checked against the reference's own step on the CPU,
tests/test_kernel_refs.py).

Why: the whole-model tests decode tiny random-init models for at most ~65 positions and compare
token lists.  The second 64-key block of self_attn_step_kernel then holds one or two keys, the
rescale between blocks runs once with a factor of ~1, and the softmax is flat (see the header of
test_gpu_kernels.py): a wrong rescale, block tail or dropped key moves no token.  The ranking rule
of beam_update_kernel matters on exact ties only, which random floats never produce.

self_attn_step_kernel   every data regime of test_gpu_kernels.py at 129 and 200 positions (the
    needle at key 0, 63, 64 and the last), lengths on both sides of the 64-key blocks, random
    ancestor paths and the prompt-shaped ones; err <= 8 * e_plain + 16 fp32 ulps of max |v|,
    e_plain capped (KR.bound / KR.cap_ok, nothing new).  profiles/r22a_attn_search_error_ratios.txt
    is a run of this file with WN_KERNEL_OPS_RATIOS set.  Exact: nothing outside out[n][d] and
    cache[step] changes, cache[step] is K | V of qkv bit for bit, a row's bits do not depend on
    the order of the rows or on the other rows.
cache_store_kernel, prompt_cache_store_kernel, step_embed_kernel   exact copies; e * scale + p
    within one rounding of the product plus one of the sum.
beam_init*_kernel, beam_update_kernel, beam_finish_kernel   equal to the NumPy statements in every
    output word -- scores bit for bit -- on untied, first-step, ended, exactly tied (dyadic),
    out-of-range-token and NaN inputs, N on both sides of the strided path (N * N > 1024 threads
    from N = 33).  A NaN candidate ranks as -inf (deviations).

Output buffers start as PATTERN; whatever no kernel owns must still hold it.
"""
import ctypes

import numpy as np
import pytest
import torch

import kernel_refs as KR
from test_gpu_kernels import PATTERN, _L, record

pytestmark = pytest.mark.gpu

assert PATTERN == KR.FILL


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pat(*shape):
    return torch.full(shape, PATTERN, dtype=torch.int32).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------
# the self-attention step

_REFS = {}


def _step_refs(key, make):
    if key not in _REFS:
        if len(_REFS) > 6:
            _REFS.clear()
        case = make()
        _REFS[key] = (case, ) + KR.self_step_refs(case)
    return _REFS[key]


def run_self_step(qkv, cache, path, H, step):
    """wn_op_attn_self_step on host tensors qkv (n, 3d), cache (max_len, n, 2d), path (n,
    max_len).  Returns out (n, d) fp32.  Asserts the exact conditions: the guard rows behind out
    keep the pattern, the cache changes in cache[step] only, and cache[step] = K | V of qkv."""
    _lib, L = _L()
    n, d = qkv.shape[0], H * 64
    max_len = path.shape[1]
    dq, dc, dp = qkv.contiguous().cuda(), cache.contiguous().cuda(), path.contiguous().cuda()
    out = _pat(n + 3, d)
    _lib.check(L.wn_op_attn_self_step(dq.data_ptr(), d, H, n, dc.data_ptr(), step, dp.data_ptr(),
                                      max_len, out.data_ptr(), _stream()), 'attn_self_step')
    torch.cuda.synchronize()
    oc, cc = out.cpu(), dc.cpu()
    assert bool((oc[n:] == PATTERN).all()), 'a store behind the n x d block of out'
    keep = torch.ones(max_len, dtype=torch.bool)
    keep[step] = False
    assert torch.equal(_bits(cc[keep]), _bits(cache[keep])), 'a store outside cache[step]'
    assert torch.equal(_bits(cc[step]), _bits(qkv[:, d:])), 'cache[step] is not K | V of qkv'
    return oc[:n].view(torch.float32)


def check_self_step(name, key, make):
    case, ref, e_plain, scale, w = _step_refs(key, make)
    out = run_self_step(case['qkv'], case['cache'], case['path'], case['H'], case['step'])
    assert torch.isfinite(out).all(), name
    record(name, (out.double() - ref).abs().max().item(), e_plain, scale)
    return case, out, w


# every H, n and length at least once; lengths on both sides of one and two 64-key blocks
STEP_SHAPES = [(1, 1, 1), (4, 5, 2), (6, 30, 63), (1, 5, 64), (4, 30, 65), (6, 1, 128),
               (4, 1, 129), (1, 30, 129), (6, 30, 200), (4, 5, 200)]


@pytest.mark.parametrize('H,n,length', STEP_SHAPES)
def test_self_step_shapes(H, n, length):
    regimes = [('unit', None)] if length == 1 else [('unit', None), ('peaked', 10.0)]
    for regime, param in regimes:
        make = lambda: KR.make_self_step_case(regime, param, H=H, n=n, length=length,
                                              seed=H + n + length)
        check_self_step(f'self_step[h{H}-n{n}-len{length}-{regime}]',
                        ('shape', H, n, length, regime), make)


@pytest.mark.parametrize('length', [129, 200])
@pytest.mark.parametrize('regime', KR.SELF_STEP_REGIMES, ids=lambda r: f'{r[0]}-{r[1]}')
def test_self_step_regimes(regime, length):
    make = lambda: KR.make_self_step_case(regime[0], regime[1], H=4, n=5, length=length, seed=51)
    _, _, w = check_self_step(f'self_step_regimes[{regime[0]}-{regime[1]}-len{length}]',
                              ('regime', regime, length), make)
    if regime in KR.SELF_STEP_NON_FLAT:
        share = (w > 0.5).double().mean().item()
        assert share >= KR.SELF_STEP_NON_FLAT[regime], (regime, share)


@pytest.mark.parametrize('length', [65, 129])
def test_self_step_prompt_paths(length):
    """6 utterances x 5 hypotheses behind a prompt of 3: positions 0..2 in the utterance's first
    slot, the later ones in slots of the utterance."""
    make = lambda: KR.make_self_step_case('peaked', 10.0, H=4, n=30, length=length, seed=61,
                                          beam=5, prompt=3)
    case, _, _ = check_self_step(f'self_step_prompt[len{length}]', ('prompt', length), make)
    first = torch.arange(30) // 5 * 5
    assert bool((case['path'][:, :3] == first.unsqueeze(1)).all())
    assert bool((case['path'] // 5 == (first // 5).unsqueeze(1)).all())


@pytest.mark.parametrize('regime', [('peaked', 10.0), ('ascending', 1.0)],
                         ids=lambda r: f'{r[0]}-{r[1]}')
def test_self_step_rows_do_not_depend_on_their_neighbours(regime):
    """The same hypotheses in another slot order (paths renamed), and one hypothesis alone in an
    n = 1 layout that names the same ancestors: the bits of a row do not change."""
    make = lambda: KR.make_self_step_case(regime[0], regime[1], H=4, n=5, length=129, seed=51)
    case, out, _ = check_self_step(f'self_step_perm[{regime[0]}]', ('regime', regime, 129), make)
    n, step = case['n'], case['step']
    perm = torch.tensor([3, 0, 4, 2, 1])                  # new slot i <- old slot perm[i]
    inv = torch.empty(n, dtype=torch.long)
    inv[perm] = torch.arange(n)
    path2 = inv[case['path'][perm].long()].to(torch.int32)
    out2 = run_self_step(case['qkv'][perm], case['cache'][:, perm], path2, case['H'], step)
    assert torch.equal(_bits(out2), _bits(out[perm]))
    for r in (0, 3):
        cache1 = case['cache'][torch.arange(case['max_len']),
                               case['path'][r].long()].unsqueeze(1).clone()
        # (columns past `step` of the path are arbitrary slots: those cache steps hold poison)
        out1 = run_self_step(case['qkv'][r:r + 1], cache1,
                             torch.zeros(1, case['max_len'], dtype=torch.int32), case['H'], step)
        assert torch.equal(_bits(out1[0]), _bits(out[r])), r


# ---------------------------------------------------------------------------------------------
# embedding of the newest token, prompt prefill -> cache


@pytest.mark.parametrize('d', [64, 260, 1280])
def test_step_embed(d):
    """x[r] = emb[last_tok[r]] * scale + pe[pos]: one rounding when the product is fused into
    the sum, two when it is not."""
    _lib, L = _L()
    rng = np.random.default_rng(d)
    V, max_pos, n, pos = 37, 9, 7, 5
    emb = rng.standard_normal((V, d)).astype(np.float32)
    pe = rng.standard_normal((max_pos, d)).astype(np.float32)
    tok = np.array([0, V - 1, 5, 5, 36, 1, 20], np.int32)
    scale = np.float32(np.sqrt(d))
    x = _pat(n + 2, d)
    de, dp, dt = _dev(emb), _dev(pe), _dev(tok)
    _lib.check(L.wn_op_attn_step_embed(dt.data_ptr(), pos, de.data_ptr(), V, dp.data_ptr(), max_pos,
                                       float(scale), d, n, x.data_ptr(), _stream()), 'step_embed')
    torch.cuda.synchronize()
    xc = x.cpu()
    assert bool((xc[n:] == PATTERN).all())
    got = xc[:n].view(torch.float32).numpy().astype(np.float64)
    prod = emb[tok].astype(np.float64) * float(scale)
    ref = prod + pe[pos].astype(np.float64)
    tol = 0.5 * np.spacing(np.abs(prod).astype(np.float32)).astype(np.float64) + \
        0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got - ref) <= tol), float(np.max(np.abs(got - ref) / tol))


def test_prompt_cache_store():
    """K | V of prefill row b * P + j lands in cache[j][b * N], bit for bit; nothing else moves."""
    _lib, L = _L()
    B, P, N, d = 3, 4, 5, 128
    qkv = torch.randn(B * P, 3 * d, generator=torch.Generator().manual_seed(5))
    dq = qkv.cuda()
    cache = _pat(P + 1, B * N, 2 * d)
    _lib.check(L.wn_op_attn_prompt_cache(dq.data_ptr(), d, B, P, N, cache.data_ptr(), _stream()),
               'prompt_cache')
    torch.cuda.synchronize()
    want = torch.full((P + 1, B * N, 2 * d), PATTERN, dtype=torch.int32)
    for b in range(B):
        for j in range(P):
            want[j, b * N] = _bits(qkv[b * P + j, d:])
    assert torch.equal(cache.cpu(), want)


# ---------------------------------------------------------------------------------------------
# the beam state

STATE_KEYS = ('score', 'end', 'tok', 'path', 'last_tok')


def _new_state_buffers(BN, max_len):
    return dict(score=_pat(BN), end=_pat(BN), tok=_pat(BN, max_len), path=_pat(BN, max_len))


def _state_to_dev(st):
    return dict(score=_dev(st['score']), end=_dev(st['end']), tok=_dev(st['tok']),
                path=_dev(st['path']))


def _assert_state(got, want, keys=STATE_KEYS, what=''):
    for k in keys:
        g = got[k].cpu().numpy()
        w = want[k].view(np.int32) if want[k].dtype == np.float32 else want[k]
        assert np.array_equal(g, w), (what, k)


def run_beam_update(dst, din, last_tok, topv, topi, B, N, step, max_len, eos, V, shared_row):
    _lib, L = _L()
    tv, ti = _dev(np.asarray(topv, np.float32)), _dev(np.asarray(topi, np.int32))
    done = ctypes.c_int32(-1)
    _lib.check(L.wn_op_beam_update(B, N, step, max_len, eos, V, tv.data_ptr(), ti.data_ptr(),
                                   din['score'].data_ptr(), din['end'].data_ptr(),
                                   din['tok'].data_ptr(), din['path'].data_ptr(),
                                   dst['score'].data_ptr(), dst['end'].data_ptr(),
                                   dst['tok'].data_ptr(), dst['path'].data_ptr(),
                                   last_tok.data_ptr(), int(shared_row), ctypes.byref(done),
                                   _stream()), 'beam_update')
    torch.cuda.synchronize()
    return done.value


def update_once(st, topv, topi, B, N, step, eos, V, shared_row):
    """One wn_op_beam_update from a host state; returns (outputs as device tensors, done)."""
    BN, max_len = st['tok'].shape
    din, dst, last = _state_to_dev(st), _new_state_buffers(BN, max_len), _pat(BN)
    done = run_beam_update(dst, din, last, topv, topi, B, N, step, max_len, eos, V, shared_row)
    dst['last_tok'] = last
    return dst, done


FAMILIES = ['untied', 'first', 'some_ended', 'all_ended', 'dup', 'bad_tokens', 'nan_parent',
            'nan_utt']
BAD_TOKENS = [-1, None, 0x7fffffff]        # None: V
# families whose candidates tie exactly for every N > 1 (-inf slots, ended parents, NaN rows)
TIED_FAMILIES = ('first', 'all_ended', 'nan_parent', 'nan_utt')


def make_update_inputs(family, B, N, step, rng, V, eos):
    """(state, topv, topi) of one family; token / path columns from `step` on hold garbage that
    no output may show."""
    BN, max_len = B * N, step + 3
    tok = rng.integers(0, V, (BN, max_len)).astype(np.int32)
    path = (np.arange(BN)[:, None] // N * N + rng.integers(0, N, (BN, max_len))).astype(np.int32)
    tok[:, step:] = -5
    path[:, step:] = -7
    score = (-rng.uniform(0.0, 20.0, BN)).astype(np.float32)
    end = np.zeros(BN, np.int32)
    topv = -np.sort(rng.uniform(0.05, 9.0, (BN, N)), axis=1).astype(np.float32)
    topi = np.stack([rng.choice(V, N, replace=False) for _ in range(BN)]).astype(np.int32)
    if family == 'first':
        score = np.where(np.arange(BN) % N == 0, 0.0, -np.inf).astype(np.float32)
    elif family == 'some_ended':
        end = (rng.random(BN) < 0.4).astype(np.int32)
        end[0] = 1
    elif family == 'all_ended':
        end[:] = 1
    elif family == 'dup':
        # quarters: every sum is exact, the N * N candidates take ~40 values, parents repeat
        score = (-rng.integers(0, 8, BN) / 4.0).astype(np.float32)
        topv = -np.sort(rng.integers(0, 6, (BN, N)) / 4.0, axis=1).astype(np.float32)
        end = (rng.random(BN) < 0.2).astype(np.int32)
    elif family == 'bad_tokens':
        for r in range(BN):
            bad = BAD_TOKENS[r % 3]
            topi[r, rng.integers(N)] = V if bad is None else bad
    elif family == 'nan_parent':
        for b in range(B):
            r = b * N + int(rng.integers(N))
            topv[r], topi[r] = np.nan, 0x7fffffff
    elif family == 'nan_utt':
        topv[:N], topi[:N] = np.nan, 0x7fffffff
    return dict(score=score, end=end, tok=tok, path=path), topv, topi


def _tied(st, topv, N):
    """True when two of an utterance's candidates are equal (NaN counted as -inf)."""
    ended = st['end'] != 0
    lp = topv.copy()
    lp[ended, 1:] = -np.inf
    lp[ended, 0] = 0.0
    with np.errstate(invalid='ignore'):
        cand = np.nan_to_num((st['score'][:, None] + lp), nan=-np.inf).reshape(-1, N * N)
    srt = np.sort(cand, axis=1)
    return bool((srt[:, 1:] == srt[:, :-1]).any())


@pytest.mark.parametrize('N', [1, 2, 3, 10, 32, 33, 64])
def test_beam_update(N):
    """Every family x (B, step, shared_row): every output word equals the NumPy statement."""
    rng = np.random.default_rng(N)
    V, eos = 2 * N + 7, 2
    for B, step, shared in ((1, 1, 0), (3, 2, 1), (3, 40, 0), (1, 40, 1), (3, 1, 1)):
        for family in FAMILIES:
            st, topv, topi = make_update_inputs(family, B, N, step, rng, V, eos)
            if family == 'untied':
                # (4096 fp32 sums of a few units do collide now and then: draw again)
                for _ in range(200):
                    if not _tied(st, topv, N):
                        break
                    st, topv, topi = make_update_inputs(family, B, N, step, rng, V, eos)
                assert not _tied(st, topv, N)
            elif (N > 1 and family in TIED_FAMILIES) or (N >= 4 and family == 'dup'):
                # (dup: N * N candidates on the 13 sums of two small multiples of 1 / 4)
                assert _tied(st, topv, N), family
            want, want_done = KR.ref_beam_update(st, topv, topi, B, N, step, eos, V, bool(shared))
            got, done = update_once(st, topv, topi, B, N, step, eos, V, shared)
            _assert_state(got, want, what=(family, B, step, shared))
            assert done == want_done, (family, B, step, shared)
            if family == 'nan_utt':
                assert bool(np.isneginf(want['score'][:N]).all()) and want['end'][:N].all()
                assert np.array_equal(want['tok'][:N, :step], st['tok'][[0] * N, :step])


@pytest.mark.parametrize('N', [3, 33])
def test_beam_update_clean_utterance_ignores_a_nan_neighbour(N):
    """Utterance 1 of 3 all NaN, or clean: utterances 0 and 2 come out the same, bit for bit."""
    rng = np.random.default_rng(N)
    B, step, V, eos = 3, 2, 2 * N + 7, 2
    st, topv, topi = make_update_inputs('untied', B, N, step, rng, V, eos)
    clean, done_clean = update_once(st, topv, topi, B, N, step, eos, V, 0)
    tv, ti = topv.copy(), topi.copy()
    tv[N:2 * N], ti[N:2 * N] = np.nan, 0x7fffffff
    dirty, done_dirty = update_once(st, tv, ti, B, N, step, eos, V, 0)
    want, want_done = KR.ref_beam_update(st, tv, ti, B, N, step, eos, V)
    _assert_state(dirty, want)
    assert done_dirty == want_done
    rows = np.r_[0:N, 2 * N:3 * N]
    for k in STATE_KEYS:
        assert np.array_equal(clean[k].cpu().numpy()[rows], dirty[k].cpu().numpy()[rows]), k
    ended_clean = int(clean['end'].cpu().numpy()[N:2 * N].sum())
    assert done_dirty - done_clean == N - ended_clean


def run_beam_init(B, N, max_len, sos, prompt):
    _lib, L = _L()
    BN = B * N
    bufs, last = _new_state_buffers(BN, max_len), _pat(BN)
    dp = _dev(np.asarray(prompt, np.int32)) if prompt is not None else None
    P = 0 if prompt is None else np.asarray(prompt).shape[1]
    _lib.check(L.wn_op_beam_init(B, N, max_len, sos, dp.data_ptr() if dp is not None else None,
                                 P, bufs['score'].data_ptr(), bufs['end'].data_ptr(),
                                 bufs['tok'].data_ptr(), bufs['path'].data_ptr(),
                                 last.data_ptr(), _stream()), 'beam_init')
    torch.cuda.synchronize()
    bufs['last_tok'] = last
    return bufs


def run_beam_finish(score, tok, B, N, length, max_len, eos, length_penalty, prefix):
    """score / tok: device tensors.  Returns (out_tok (B, max_len), out_len (B)) as NumPy."""
    _lib, L = _L()
    out_tok, out_len = _pat(B, max_len), _pat(B)
    _lib.check(L.wn_op_beam_finish(B, N, length, max_len, eos, float(length_penalty),
                                   score.data_ptr(), tok.data_ptr(), out_tok.data_ptr(),
                                   out_len.data_ptr(), prefix, _stream()), 'beam_finish')
    torch.cuda.synchronize()
    return out_tok.cpu().numpy(), out_len.cpu().numpy()


@pytest.mark.parametrize('prefix', [1, 4])
@pytest.mark.parametrize('length_penalty', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('N', [1, 10, 64])
def test_beam_finish(N, length_penalty, prefix):
    """The draws of test_kernel_refs.test_ref_beam_finish_matches_reference (none rejected: the
    fp64 winner leads by more than 4 fp32 ulps, so the last place of powf decides nothing)."""
    B, eos = 3, 2
    score, tok, length = KR.make_beam_finish_case(B, N, prefix, seed=N + prefix, eos=eos)
    s = KR.beam_finish_scores(score, tok, B, N, length, eos, length_penalty)
    assert all(KR.beam_finish_margin_ok(s[b]) for b in range(B))
    want_tok, want_len, _ = KR.ref_beam_finish(score, tok, B, N, length, eos, length_penalty,
                                               prefix)
    got_tok, got_len = run_beam_finish(_dev(score), _dev(tok), B, N, length, tok.shape[1], eos,
                                       length_penalty, prefix)
    assert np.array_equal(got_len, want_len) and np.array_equal(got_tok, want_tok)


@pytest.mark.parametrize('length_penalty', [0.0, 0.3, 1.0])
def test_beam_finish_edges(length_penalty):
    """Two best rows with the same score and count but other tokens: the first wins.  sos == eos and nothing else in any row (count 0):
    row 0 with length 0."""
    B, N, eos, length, max_len = 2, 10, 2, 6, 8
    rng = np.random.default_rng(3)
    tok = rng.integers(3, 40, (B * N, max_len)).astype(np.int32)
    tok[:, 0] = eos                                   # <sos> = <eos>
    score = (-rng.uniform(5.0, 9.0, B * N)).astype(np.float32)
    for b, (i, j) in enumerate(((2, 7), (0, 9))):     # rows i < j of utterance b: tied, best
        # the same score and the same count (the same fp32 quotient), other tokens
        tok[b * N + j, 1:] = (tok[b * N + i, 1:] - 2) % 37 + 3
        score[b * N + i] = score[b * N + j] = -1.0
    s = KR.beam_finish_scores(score, tok, B, N, length, eos, length_penalty)
    assert KR.beam_finish_margin_ok(s[0], same=(7, )) and KR.beam_finish_margin_ok(s[1], same=(9, ))
    want_tok, want_len, best = KR.ref_beam_finish(score, tok, B, N, length, eos, length_penalty)
    assert best.tolist() == [2, 0]
    assert not np.array_equal(tok[7, 1:length], tok[2, 1:length])
    got_tok, got_len = run_beam_finish(_dev(score), _dev(tok), B, N, length, max_len, eos,
                                       length_penalty, 1)
    assert np.array_equal(got_len, want_len) and np.array_equal(got_tok, want_tok)
    # count 0 in every row: [sos, eos, eos, ...]
    tok[:, :length] = eos
    want_tok, want_len, best = KR.ref_beam_finish(score, tok, B, N, length, eos, length_penalty)
    assert want_len.tolist() == [0, 0]
    if length_penalty > 0:
        assert best.tolist() == [0, 0]                # every penalised score is -inf
    got_tok, got_len = run_beam_finish(_dev(score), _dev(tok), B, N, length, max_len, eos,
                                       length_penalty, 1)
    assert np.array_equal(got_len, want_len) and np.array_equal(got_tok, want_tok)


@pytest.mark.parametrize('B,N,prompt_len', [(3, 10, 0), (1, 33, 0), (2, 4, 3)])
def test_beam_chain(B, N, prompt_len):
    """init -> 6 updates on synthetic top-k tables -> finish, the state ping-ponging between two
    device buffers as in beam_search_run: equal to the NumPy chain after every call."""
    rng = np.random.default_rng(B + N)
    V, eos, sos, steps = 2 * N + 7, 2, 1, 6
    BN = B * N
    prompt = rng.integers(3, V, (B, prompt_len)).astype(np.int32) if prompt_len else None
    first = prompt_len if prompt_len else 1
    max_len = first + steps + 2
    want = KR.ref_beam_init(B, N, max_len, sos=sos, prompt=prompt)
    cur = run_beam_init(B, N, max_len, sos, prompt)
    _assert_state(cur, want, what='init')
    last = cur.pop('last_tok')
    nxt = _new_state_buffers(BN, max_len)
    for i in range(first, first + steps):
        topv = -np.sort(rng.uniform(0.05, 3.0, (BN, N)), axis=1).astype(np.float32)
        topi = np.stack([rng.choice(V, N, replace=False) for _ in range(BN)]).astype(np.int32)
        topi[rng.random(BN) < 0.2, 0] = eos
        shared = i == prompt_len
        want, want_done = KR.ref_beam_update(want, topv, topi, B, N, i, eos, V, shared)
        done = run_beam_update(nxt, cur, last, topv, topi, B, N, i, max_len, eos, V, shared)
        cur, nxt = nxt, cur
        _assert_state(dict(cur, last_tok=last), want, what=('update', i))
        assert done == want_done
    assert want['end'].any() and not want['end'].all()
    length = first + steps
    for lp in (0.0, 0.3):
        s = KR.beam_finish_scores(want['score'], want['tok'], B, N, length, eos, lp)
        assert all(KR.beam_finish_margin_ok(s[b]) for b in range(B))
        want_tok, want_len, _ = KR.ref_beam_finish(want['score'], want['tok'], B, N, length, eos, lp,
                                                   first)
        got_tok, got_len = run_beam_finish(cur['score'], cur['tok'], B, N, length, max_len, eos, lp,
                                           first)
        assert np.array_equal(got_len, want_len) and np.array_equal(got_tok, want_tok)


# ---------------------------------------------------------------------------------------------


def test_hooks_reject_bad_arguments():
    """Refused on the host; nothing is launched."""
    _lib, L = _L()
    buf = _pat(4096)
    p, s = buf.data_ptr(), _stream()
    path = torch.zeros(2, 8, dtype=torch.int32)
    path[1, 2] = 2
    dpath = path.cuda()

    def status(rc, msg):
        assert rc == -1 and msg in L.wn_last_error().decode(), L.wn_last_error()

    status(L.wn_op_attn_self_step(None, 64, 1, 2, p, 1, dpath.data_ptr(), 8, p, s), 'null')
    status(L.wn_op_attn_self_step(p, 96, 1, 2, p, 1, dpath.data_ptr(), 8, p, s), 'heads * 64')
    status(L.wn_op_attn_self_step(p, 64, 1, 0, p, 1, dpath.data_ptr(), 8, p, s), 'n outside')
    status(L.wn_op_attn_self_step(p, 64, 1, 2, p, 8, dpath.data_ptr(), 8, p, s), 'step outside')
    status(L.wn_op_attn_self_step(p, 64, 1, 2, p, -1, dpath.data_ptr(), 8, p, s), 'step outside')
    status(L.wn_op_attn_self_step(p, 64, 1, 2, p, 2, dpath.data_ptr(), 8, p, s), 'path entry')
    tok = _dev(np.array([0, 5], np.int32))
    status(L.wn_op_attn_step_embed(tok.data_ptr(), 0, None, 6, p, 4, 1.0, 64, 2, p, s), 'null')
    status(L.wn_op_attn_step_embed(tok.data_ptr(), 4, p, 6, p, 4, 1.0, 64, 2, p, s), 'position')
    status(L.wn_op_attn_step_embed(tok.data_ptr(), 0, p, 6, p, 4, 1.0, 62, 2, p, s), 'd / n / V')
    status(L.wn_op_attn_step_embed(tok.data_ptr(), 0, p, 5, p, 4, 1.0, 64, 2, p, s), 'token outside')
    status(L.wn_op_attn_prompt_cache(p, 64, 1, 1, 65, p, s), 'beam_size')
    status(L.wn_op_attn_prompt_cache(p, 64, 1, 0, 2, p, s), 'd / B / P')
    status(L.wn_op_attn_prompt_cache(p, 64, 1, 1, 2, None, s), 'null')
    status(L.wn_op_beam_init(1, 65, 4, 1, None, 0, p, p, p, p, p, s), 'beam_size')
    status(L.wn_op_beam_init(1, 0, 4, 1, None, 0, p, p, p, p, p, s), 'beam_size')
    status(L.wn_op_beam_init(1, 2, 4, 1, p, 5, p, p, p, p, p, s), 'prompt length')
    status(L.wn_op_beam_init(1, 2, 4, 1, None, 0, p, None, p, p, p, s), 'null')
    done = ctypes.c_int32(0)

    def upd(N=2, step=1, max_len=4, eos=2, V=9, topv=p, done=done):
        return L.wn_op_beam_update(1, N, step, max_len, eos, V, topv, p, p, p, p, p, p, p, p, p, p,
                                   0, ctypes.byref(done) if done is not None else None, s)

    status(upd(N=65), 'beam_size')
    status(upd(N=0), 'beam_size')
    status(upd(step=0), 'step outside')
    status(upd(step=4), 'step outside')
    status(upd(V=0), 'eos outside')
    status(upd(eos=9), 'eos outside')
    status(upd(eos=-1), 'eos outside')
    status(upd(topv=None), 'null')
    status(upd(done=None), 'null')
    status(L.wn_op_beam_finish(1, 65, 2, 4, 2, 0.0, p, p, p, p, 1, s), 'beam_size')
    status(L.wn_op_beam_finish(1, 2, 5, 4, 2, 0.0, p, p, p, p, 1, s), 'prefix <= len')
    status(L.wn_op_beam_finish(1, 2, 2, 4, 2, 0.0, p, p, p, p, 3, s), 'prefix <= len')
    status(L.wn_op_beam_finish(1, 2, 2, 4, 2, 0.0, p, None, p, p, 1, s), 'null')
    torch.cuda.synchronize()
    assert bool((buf.cpu() == PATTERN).all())
