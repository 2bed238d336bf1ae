"""The RNN-T prefix beam search on the GPU (csrc/transducer_beam.hip, csrc/cabi_transducer.hip):
 (a) wn_op_joint_fuse_topk against fp64 NumPy (tests/transducer_beam_formulation.ref_fuse_topk);
 (b) wn_op_rnnt_beam_step on the hand-written cases and on random chains against ref_beam_step;
 (c) the search on the reference's recorded encoder output against the reference's recorded
     final beams (tests/golden/rnnt/rnnt_beam_tiny.npz, tools/gen_golden_transducer_beam.py);
 (d) a vocabulary of 8329 against the fp64 restatement;
 (e) Transducer.beam_search / decode end to end.

Error bars.  (a): the kernel's max-abs error of the fused values against fp64 may be 4 x the error
of the same rows by torch in fp32 on the CPU against fp64, plus 1e-6 (the project's rule; the 4
covers another summation order); indices must equal the fp64 top-k wherever the fp64 gaps to
both neighbours at that rank exceed twice that bar.  (c): scores within 4 e_score + 1e-6 of the
fp64 reference, e_score being the fixture's measured error of the fp32 reference's scores; the
fixture's decision gaps are at least twice that.  The measured ratios are printed."""
import json
import math
import os

import numpy as np
import pytest
import torch

import transducer_beam_formulation as BF
import transducer_formulation as TF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [(0.3, 0.7), (0.0, 1.0), (1.0, 0.0)]


def _lib():
    from wenet_amd import _lib as L
    return L, L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- (a) joint + fusion + top-k ---------------------------------------------------------------
N_ENC, N_PRED = 40, 5


def _fuse_case(J, V, seed):
    g = torch.Generator().manual_seed(seed)
    enc_proj = torch.randn(N_ENC, J, generator=g)
    pred_proj = torch.randn(N_PRED, J, generator=g)
    W = torch.randn(V, J, generator=g) * (3.0 / math.sqrt(J))
    bias = torch.randn(V, generator=g) * 0.1
    ctc = torch.log_softmax(torch.randn(N_ENC, V, generator=g) * 3.0, dim=-1)
    # identical ffn_out rows (and CTC columns) that rank high: exact ties inside one wave's 32
    # columns, across two waves of a block and (V > 128) across column blocks
    pairs = [(5, 9), (3, 40)] + ([(7, V - 100)] if V > 256 else [])
    if V > 64 * 128:
        pairs.append((130, 64 * 128 + 2))
    for n, (i, j) in enumerate(pairs):
        W[j] = W[i]
        bias[i] = bias[j] = 2.0 + n
        ctc[:, j] = ctc[:, i]
    return enc_proj, pred_proj, W, bias, ctc, pairs


def _fuse_run(L, dev, row_enc, row_pred, J, V, cw, tw, k, want_rows=True, row_ctc=None):
    Lm, _ = _lib()
    enc_proj, pred_proj, W, bias, ctc = dev
    M = len(row_enc)
    re_ = np.ascontiguousarray(row_enc, dtype=np.int32)
    rp_ = np.ascontiguousarray(row_pred, dtype=np.int32)
    rc_ = None if row_ctc is None else np.ascontiguousarray(row_ctc, dtype=np.int32)
    val = np.full((M, k), 7.5, dtype=np.float32)
    idx = np.full((M, k), -7, dtype=np.int32)
    rows = np.full((M, V), 7.5, dtype=np.float32) if want_rows else None
    st = L.wn_op_joint_fuse_topk(enc_proj.data_ptr(), N_ENC, pred_proj.data_ptr(), N_PRED,
                                 Lm.i32p(re_), Lm.i32p(rp_), W.data_ptr(), bias.data_ptr(), M, J,
                                 V, ctc.data_ptr() if cw != 0 else None, N_ENC,
                                 None if rc_ is None else Lm.i32p(rc_), cw, tw, k, Lm.f32p(val),
                                 Lm.i32p(idx), None if rows is None else Lm.f32p(rows), _stream())
    assert st == 0, L.wn_last_error()
    return val, idx, rows


def _fused64(case, row_enc, row_pred, cw, tw, dtype):
    """The fused rows of the live rows by torch on the CPU in `dtype`, as fp64 arrays."""
    enc_proj, pred_proj, W, bias, ctc, _ = [t.to(dtype) if torch.is_tensor(t) else t for t in case]
    with torch.no_grad():
        logp = torch.log_softmax(torch.tanh(enc_proj[row_enc] + pred_proj[row_pred]) @ W.T + bias,
                                 dim=-1)
        # prefix_beam_search.py:99-101 as written
        f = torch.log(torch.add(tw * torch.exp(logp), cw * torch.exp(ctc[row_enc])))
    return f.double().numpy()


@pytest.mark.parametrize('M', [3, 48, 130])
@pytest.mark.parametrize('J,V', [(160, 67), (512, 4233), (32, 8329)])
def test_joint_fuse_topk_against_fp64(J, V, M):
    _, L = _lib()
    case = _fuse_case(J, V, seed=J + V)
    pairs = case[5]
    rng = np.random.default_rng(M * 7 + J)
    row_enc = rng.integers(0, N_ENC, size=M)
    row_pred = rng.integers(0, N_PRED, size=M)
    row_enc[rng.random(M) < 0.2] = -1          # empty slots / finished utterances
    row_enc[0], row_enc[M - 1] = 11, -1
    live = row_enc >= 0
    dev = tuple(t.cuda().contiguous() for t in case[:5])
    lower = {j: i for i, j in pairs}
    ties = 0
    for cw, tw in WEIGHTS:
        ref = _fused64(case, row_enc[live], row_pred[live], cw, tw, torch.float64)
        plain = _fused64(case, row_enc[live], row_pred[live], cw, tw, torch.float32)
        assert np.isfinite(ref).all()
        e_plain = np.abs(plain - ref).max()
        bar = 4 * e_plain + 1e-6
        order = np.argsort(-ref, axis=1, kind='stable')
        for k in (1, 5, 16):
            val, idx, rows = _fuse_run(L, dev, row_enc, row_pred, J, V, cw, tw, k)
            assert (idx[~live] == -1).all() and np.isneginf(val[~live]).all()
            assert (rows[~live] == 0).all()
            got = rows[live].astype(np.float64)
            err = np.abs(got - ref).max()
            print(f'fuse_topk J={J} V={V} M={M} w=({cw}, {tw}) k={k}: err {err:.3e}, torch fp32 '
                  f'{e_plain:.3e}, ratio {err / max(e_plain, 1e-30):.2f}')
            assert err <= bar, (err, e_plain)
            gi, gv = idx[live], val[live]
            assert ((gi >= 0) & (gi < V)).all()
            checked = 0
            for r in range(gi.shape[0]):
                assert len(set(gi[r].tolist())) == k
                # the values are those of the row, in descending order, ties by index
                assert np.array_equal(gv[r].view(np.int32), rows[live][r][gi[r]].view(np.int32))
                assert all(gv[r][i] > gv[r][i + 1] or (gv[r][i] == gv[r][i + 1] and gi[r][i] < gi[r][i + 1])
                           for i in range(k - 1))
                # nothing outside the top-k beats its last entry
                rest = np.delete(rows[live][r], gi[r])
                assert rest.max() <= gv[r][-1]
                s = ref[r][order[r]]
                for i in range(k):
                    up = s[i - 1] - s[i] if i > 0 else np.inf
                    down = s[i] - s[i + 1]
                    if min(up, down) > 2 * bar:
                        assert gi[r][i] == order[r][i], (r, i, gi[r][i], order[r][i], up, down)
                        checked += 1
                for pos, c in enumerate(gi[r].tolist()):
                    if c in lower:         # the duplicate: its lower twin sits right before it
                        assert pos > 0 and gi[r][pos - 1] == lower[c], (r, gi[r].tolist())
                        ties += 1
            assert checked >= gi.size // 2, (checked, gi.size)
    if M >= 48:
        assert ties >= 1
    # permuted rows and a row alone (M = 1): the same bits for that row; a CTC row map of its own
    cw, tw, k = 0.3, 0.7, 5
    val, idx, rows = _fuse_run(L, dev, row_enc, row_pred, J, V, cw, tw, k)
    perm = rng.permutation(M)
    val_p, idx_p, rows_p = _fuse_run(L, dev, row_enc[perm], row_pred[perm], J, V, cw, tw, k)
    assert np.array_equal(idx_p, idx[perm])
    assert np.array_equal(val_p.view(np.int32), val[perm].view(np.int32))
    assert np.array_equal(rows_p.view(np.int32), rows[perm].view(np.int32))
    for m in (0, M // 2, M - 2):
        v1, i1, r1 = _fuse_run(L, dev, row_enc[m:m + 1], row_pred[m:m + 1], J, V, cw, tw, k)
        assert np.array_equal(i1[0], idx[m]) and np.array_equal(r1.view(np.int32)[0],
                                                                rows.view(np.int32)[m]), m
    v2, i2, _ = _fuse_run(L, dev, row_enc, row_pred, J, V, cw, tw, k, False,
                          row_ctc=np.maximum(row_enc, 0))
    assert np.array_equal(i2, idx) and np.array_equal(v2.view(np.int32), val.view(np.int32))


def test_joint_fuse_topk_refuses_rows_outside_its_matrices():
    _, L = _lib()
    case = _fuse_case(160, 67, seed=1)
    dev = tuple(t.cuda().contiguous() for t in case[:5])
    Lm, _ = _lib()
    for row_enc, row_pred, row_ctc, what in (([N_ENC], [0], None, b'row map'),
                                             ([0], [N_PRED], None, b'row map'),
                                             ([0], [-1], None, b'row map'),
                                             ([0], [0], [N_ENC], b'CTC row map'),
                                             ([0], [0], [-1], b'CTC row map')):
        re_, rp_ = np.array(row_enc, dtype=np.int32), np.array(row_pred, dtype=np.int32)
        rc_ = None if row_ctc is None else np.array(row_ctc, dtype=np.int32)
        val, idx = np.zeros((1, 2), np.float32), np.zeros((1, 2), np.int32)
        st = L.wn_op_joint_fuse_topk(dev[0].data_ptr(), N_ENC, dev[1].data_ptr(), N_PRED,
                                     Lm.i32p(re_), Lm.i32p(rp_), dev[2].data_ptr(),
                                     dev[3].data_ptr(), 1, 160, 67, dev[4].data_ptr(), N_ENC,
                                     None if rc_ is None else Lm.i32p(rc_), 0.3, 0.7, 2,
                                     Lm.f32p(val), Lm.i32p(idx), None, _stream())
        assert st == -1 and what in L.wn_last_error(), (row_enc, row_pred, row_ctc)


# ---- (b) the beam step --------------------------------------------------------------------------
def _pack(slots, beam, max_tok):
    B = len(slots)
    n_live = np.array([len(u) for u in slots], dtype=np.int32)
    scores = np.full((B, beam), -np.inf, dtype=np.float64)
    tok_lens = np.zeros((B, beam), dtype=np.int32)
    tokens = np.full((B, beam, max_tok), -1, dtype=np.int32)
    for b, u in enumerate(slots):
        for j, (hyp, s) in enumerate(u):
            scores[b, j], tok_lens[b, j] = s, len(hyp)
            tokens[b, j, :len(hyp)] = hyp
    return n_live, scores, tok_lens, tokens


def _pack_top(top_val, top_idx, B, beam):
    tv = np.full((B, beam, beam), -np.inf, dtype=np.float32)
    ti = np.zeros((B, beam, beam), dtype=np.int32)
    for b in range(B):
        if top_val[b] is None:
            continue
        for j in range(len(top_val[b])):
            tv[b, j], ti[b, j] = top_val[b][j], top_idx[b][j]
    return tv, ti


def _step_run(L, slots, top_val, top_idx, frame, lens, blank, beam, V, max_tok):
    Lm, _ = _lib()
    B = len(slots)
    n_live, scores, tok_lens, tokens = _pack(slots, beam, max_tok)
    tv, ti = _pack_top(top_val, top_idx, B, beam)
    ln = np.array(lens, dtype=np.int32)
    o_n = np.full((B, ), -7, dtype=np.int32)
    o_sc = np.zeros((B, beam), dtype=np.float64)
    o_len = np.full((B, beam), -7, dtype=np.int32)
    o_tok = np.full((B, beam, max_tok), -7, dtype=np.int32)
    maps = [np.full((B, beam), -7, dtype=np.int32) for _ in range(4)]
    st = L.wn_op_rnnt_beam_step(B, beam, blank, V, frame, Lm.i32p(ln), max_tok, Lm.i32p(n_live),
                                Lm.f64p(scores), Lm.i32p(tok_lens), Lm.i32p(tokens), Lm.f32p(tv),
                                Lm.i32p(ti), Lm.i32p(o_n), Lm.f64p(o_sc), Lm.i32p(o_len),
                                Lm.i32p(o_tok), *[Lm.i32p(m) for m in maps], _stream())
    assert st == 0, L.wn_last_error()
    out = [[(o_tok[b, j, :o_len[b, j]].tolist(), float(o_sc[b, j])) for j in range(o_n[b])]
           for b in range(B)]
    # beyond the live slots: empty
    for b in range(B):
        assert np.isneginf(o_sc[b, o_n[b]:]).all() and (o_len[b, o_n[b]:] == 0).all()
    return (out, *maps)


def _same_step(got, want, fused=None):
    """Every output word equal; scores bit for bit where no fusion happened, within 4 fp64 ulps
    where one did (fused[b][j]; None: the hand-written cases, whose fused entries were worked
    out with another log / exp)."""
    g_slots, w_slots = got[0], want[0]
    assert [[h for h, _ in u] for u in g_slots] == [[h for h, _ in u] for u in w_slots]
    for b, (gu, wu) in enumerate(zip(g_slots, w_slots)):
        for j, ((_, a), (_, c)) in enumerate(zip(gu, wu)):
            ulps = 4 if fused is None or fused[b][j] else 0
            assert BF.same_score(a, c, ulps), (b, j, a, c, ulps)
    for g, w in zip(got[1:], want[1:]):
        assert np.array_equal(np.asarray(g), np.asarray(w)), (g, w)


@pytest.mark.parametrize('case', BF.hand_cases(), ids=lambda c: c['name'])
def test_beam_step_hand_cases(case):
    _, L = _lib()
    slots = case['slots']
    for i, f in enumerate(case['frames']):
        got = _step_run(L, slots, f['top_val'], f['top_idx'], case['frame0'] + i, case['lens'], 0,
                        case['beam'], 16, 6)
        _same_step(got, (f['want'], f['src'], f['tok'], f['advance'], f['row_enc']))
        slots = f['want']


def _random_chain(L, beam, seed, frames=12):
    rng = np.random.default_rng(seed)
    V = max(beam + 2, 6)             # a small vocabulary: prefixes meet again all the time
    lens = [frames, 7, 0, frames - 1]
    slots = [[([], 0.0)] for _ in lens]
    n_fused = n_ties = 0
    for i in range(frames):
        top_val, top_idx = [], []
        for b, u in enumerate(slots):
            if i >= lens[b]:
                top_val.append(None)
                top_idx.append(None)
                continue
            tv, ti = [], []
            lasts = sorted({h[-1] for h, _ in u if h})
            for _ in u:
                # multiples of 1/4: exact score ties happen; now and then a -inf or a NaN
                v = -np.sort(rng.integers(0, 12, size=beam)).astype(np.float32) / 4
                r = rng.random()
                if r < 0.08:
                    v[-1] = -np.inf
                elif r < 0.12:
                    v[rng.integers(0, beam)] = np.nan
                tv.append(v.tolist())
                # mostly: blank and the last tokens of the live hypotheses first, so that a
                # hypothesis and its parent meet in one list (a fusion)
                first = [0] + lasts if rng.random() < 0.7 else []
                pick = list(dict.fromkeys(first + rng.permutation(V).tolist()))[:beam]
                ti.append(rng.permutation(pick).tolist())
            top_val.append(tv)
            top_idx.append(ti)
        trace = []
        want = BF.ref_beam_step(slots, top_val, top_idx, i, lens, 0, beam, np.float32, trace)
        fused = [[False] * beam for _ in lens]
        for t in trace:
            fused[t['b']] = t['fused'][:beam] + [False] * beam
            n_fused += t['n_fused']
            s = [BF.rank_key(x) for x in t['sorted'][:beam + 1]]
            n_ties += sum(1 for a, c in zip(s, s[1:]) if a == c)
        got = _step_run(L, slots, top_val, top_idx, i, lens, 0, beam, V, frames)
        _same_step(got, want, fused)
        slots = want[0]
    return n_fused, n_ties


@pytest.mark.parametrize('beam', [1, 2, 5, 16])
def test_beam_step_random_chains(beam):
    _, L = _lib()
    n_fused = n_ties = 0
    for seed in range(3):
        f, t = _random_chain(L, beam, 100 * beam + seed)
        n_fused += f
        n_ties += t
    print(f'beam {beam}: {n_fused} fusions, {n_ties} tied neighbours in 3 chains of 12 frames')
    if beam > 1:
        assert n_fused >= 5 and n_ties >= 1


# ---- (c) the search on the recorded encoder output -------------------------------------------
@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_beam_tiny.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    return meta, torch.from_numpy(z['enc']).cuda(), meta['enc_lens']


@pytest.fixture(scope='module')
def model(gold):
    from wenet_amd import Transducer
    from wenet_amd import synthetic as S
    configs = S.make_configs(gold[0]['config'])
    return Transducer(configs, S.make_state_dict(configs, gold[0]['wseed']), device='cuda')


@pytest.mark.parametrize('cw,tw', WEIGHTS)
def test_search_on_the_recorded_encoder_output(gold, model, cw, tw):
    from wenet_amd.transducer import prefix_beam_search
    meta, enc, lens = gold
    bar = 4 * meta['e_score'] + 1e-6
    for beam in meta['beams']:
        run = meta['runs'][f'{cw}_{tw}_{beam}']
        want = run['fp64']
        got = prefix_beam_search(model, enc, lens, beam, cw, tw)
        assert [[t for t, _ in u] for u in got] == [[t for t, _ in u] for u in want], beam
        err = max(abs(s - r) for g, w in zip(got, want) for (_, s), (_, r) in zip(g, w))
        print(f'search ({cw}, {tw}) beam {beam}: score err {err:.3e}, e_score '
              f"{meta['e_score']:.3e}, ratio {err / meta['e_score']:.2f}")
        assert err <= bar, (beam, err, bar)
        # each utterance alone, and the batch in another order: the same lists and bits
        for b in range(len(lens)):
            assert prefix_beam_search(model, enc[b:b + 1], lens[b:b + 1], beam, cw, tw) == [got[b]]
        order = [2, 0, 1]
        again = prefix_beam_search(model, enc[order].contiguous(), [lens[b] for b in order], beam,
                                   cw, tw)
        assert again == [got[b] for b in order]


def test_search_refusals(gold, model):
    from wenet_amd.transducer import prefix_beam_search
    _, enc, lens = gold
    for beam, cw, tw, what in ((0, 0.3, 0.7, 'beam must be in'), (17, 0.3, 0.7, 'beam must be in'),
                               (5, -0.1, 0.7, 'must be >= 0'), (5, 0.3, -0.7, 'must be >= 0'),
                               (5, 0.0, 0.0, 'both 0')):
        with pytest.raises(RuntimeError, match=what):
            prefix_beam_search(model, enc, lens, beam, cw, tw)
    # an empty utterance in the batch: one empty hypothesis with score 0
    got = prefix_beam_search(model, enc, [lens[0], 0, lens[2]], 3, 0.3, 0.7)
    assert got[1] == [([], 0.0)] and len(got[0]) == 3


# ---- (d) a vocabulary of 65 x 128 + 9 ------------------------------------------------------------
# No recorded reference at this size; the fp64 restatement is the reference, and it is one only
# where fp32 cannot flip a decision.  e_row: the error of the same fused rows (the top beam + 1
# values of every live row of the fp64 path) by torch in fp32 on the CPU.  A score is a sum of one
# fused value per frame, rounded to fp32 once per frame, and log_add of two such sums does not
# amplify their errors (its two partial derivatives add up to 1), so
#     e_score <= T' (e_row + 2^-24 max|score|).
# The conditions of the golden fixture are asserted on the fp64 side: membership gaps
# >= 8 e_row + 2e-6, cut and final-beam gaps >= 8 e_score + 2e-6.
WIDE_SEED = 3      # of seeds 0..5, one that meets the conditions below and fuses a prefix
WIDE_LENS = [21, 8, 16]
WIDE_BEAM = 4


def _wide_case(wseed):
    from wenet_amd import synthetic as S
    configs = S.make_configs('tiny_rnnt_wide')
    sd = S.make_state_dict(configs, wseed)
    d = configs['encoder_conf']['output_size']
    rng = np.random.default_rng(1234)
    enc = rng.standard_normal((len(WIDE_LENS), max(WIDE_LENS), d)).astype(np.float32)
    sdn = {k: v.numpy() for k, v in sd.items()}
    W = TF.weights64(sdn, 2)
    x = enc.astype(np.float64) @ sdn['ctc.ctc_lo.weight'].astype(np.float64).T \
        + sdn['ctc.ctc_lo.bias'].astype(np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    ctc64 = x - np.log(np.exp(x).sum(axis=-1, keepdims=True))
    cw, tw = 0.3, 0.7
    trace = []
    want = BF.prefix_beam_search(enc, WIDE_LENS, ctc64, W, 0, WIDE_BEAM, cw, tw, np.float32, trace)
    # e_row by torch in fp32
    t = {k: torch.from_numpy(np.ascontiguousarray(sdn[k])) for k in
         ('joint.enc_ffn.weight', 'joint.enc_ffn.bias', 'joint.ffn_out.weight',
          'joint.ffn_out.bias', 'ctc.ctc_lo.weight', 'ctc.ctc_lo.bias')}
    e_row, gaps = 0.0, dict(member=np.inf, cut=np.inf, final=np.inf)
    top_score = 0.0
    with torch.no_grad():
        tenc = torch.from_numpy(enc)
        enc_proj = tenc @ t['joint.enc_ffn.weight'].T + t['joint.enc_ffn.bias']
        ctc32 = torch.log_softmax(tenc @ t['ctc.ctc_lo.weight'].T + t['ctc.ctc_lo.bias'], dim=-1)
        for fr in trace:
            i = fr['frame']
            for (b, j), top in fr['rows'].items():
                pp = torch.from_numpy(fr['pred_proj'][(b, j)]).float()
                logp = torch.log_softmax(torch.tanh(enc_proj[b, i] + pp) @ t['joint.ffn_out.weight'].T
                                         + t['joint.ffn_out.bias'], dim=-1)
                f = torch.log(torch.add(tw * torch.exp(logp), cw * torch.exp(ctc32[b, i])))
                f32 = torch.sort(f, descending=True)[0][:WIDE_BEAM + 1].double().numpy()
                e_row = max(e_row, float(np.abs(f32 - top).max()))
                gaps['member'] = min(gaps['member'], float(top[WIDE_BEAM - 1] - top[WIDE_BEAM]))
            for s in fr['steps']:
                srt = s['sorted']
                top_score = max(top_score, max(abs(v) for v in srt[:WIDE_BEAM + 1]))
                if len(srt) > WIDE_BEAM:
                    gaps['cut'] = min(gaps['cut'], srt[WIDE_BEAM - 1] - srt[WIDE_BEAM])
    for u in want:
        sc = [s for _, s in u]
        gaps['final'] = min([gaps['final']] + [a - c for a, c in zip(sc, sc[1:])])
    e_score = max(WIDE_LENS) * (e_row + 2.0 ** -24 * top_score)
    n_fused = sum(s['n_fused'] for fr in trace for s in fr['steps'])
    return configs, sd, enc, want, dict(e_row=e_row, e_score=e_score, n_fused=n_fused, **gaps)


def test_search_with_a_wide_vocabulary():
    from wenet_amd import Transducer
    from wenet_amd.transducer import prefix_beam_search
    configs, sd, enc, want, facts = _wide_case(WIDE_SEED)
    print('wide vocabulary case:', facts, [[len(t) for t, _ in u] for u in want])
    assert facts['member'] >= 8 * facts['e_row'] + 2e-6, facts
    assert min(facts['cut'], facts['final']) >= 8 * facts['e_score'] + 2e-6, facts
    assert facts['n_fused'] >= 1
    assert any(t >= 128 for u in want for h, _ in u for t in h)       # beyond column block 0
    model = Transducer(configs, sd, device='cuda')
    got = prefix_beam_search(model, torch.from_numpy(enc).cuda(), WIDE_LENS, WIDE_BEAM, 0.3, 0.7)
    assert [[t for t, _ in u] for u in got] == [[t for t, _ in u] for u in want]
    err = max(abs(s - r) for g, w in zip(got, want) for (_, s), (_, r) in zip(g, w))
    print(f"wide search: score err {err:.3e}, e_score bound {facts['e_score']:.3e}")
    assert err <= 4 * facts['e_score'] + 1e-6


# ---- (e) end to end ------------------------------------------------------------------------------
def test_end_to_end(gold, model):
    from wenet_amd import synthetic as S
    from wenet_amd.transducer import prefix_beam_search
    meta, _, _ = gold
    feats, flens = S.make_features(meta['batch'], tuple(meta['frames']), seed=meta['fseed'])
    feats = feats.cuda()
    enc, mask = model._forward_encoder(feats, flens)
    nbest = prefix_beam_search(model, enc, mask.squeeze(1).sum(1).cpu(), 5, 0.3, 0.7)
    toks, scores = model.beam_search(feats, flens, beam_size=5)
    assert toks == [u[0][0] for u in nbest] and scores == [u[0][1] for u in nbest]
    assert all(len(u) == 5 and all(a[1] >= c[1] for a, c in zip(u, u[1:])) for u in nbest)
    # one encoder pass serves the three searches
    modes = ['rnnt_beam_search', 'rnnt_greedy_search', 'ctc_prefix_beam_search']
    res = model.decode(modes, feats, flens, beam_size=5)
    assert sorted(res) == sorted(modes)
    for r, u in zip(res['rnnt_beam_search'], nbest):
        assert r.tokens == u[0][0] and r.score == u[0][1]
        assert r.nbest == [t for t, _ in u] and r.nbest_scores == [s for _, s in u]
    assert [r.tokens for r in res['rnnt_greedy_search']] == model.greedy_search(feats, flens)
    alone = model.decode(['ctc_prefix_beam_search'], feats, flens, beam_size=5)
    assert [list(r.tokens) for r in res['ctc_prefix_beam_search']] == \
        [list(r.tokens) for r in alone['ctc_prefix_beam_search']]
    # decode()'s own ctc_weight is the rescoring weight: this mode does not read it
    res2 = model.decode(['rnnt_beam_search'], feats, flens, beam_size=5, ctc_weight=0.9)
    assert [r.nbest for r in res2['rnnt_beam_search']] == [r.nbest for r in res['rnnt_beam_search']]
    res3 = model.decode(['rnnt_beam_search'], feats, flens, beam_size=5, search_ctc_weight=0.0,
                        search_transducer_weight=1.0)
    want3 = prefix_beam_search(model, enc, mask.squeeze(1).sum(1).cpu(), 5, 0.0, 1.0)
    assert [r.nbest_scores for r in res3['rnnt_beam_search']] == [[s for _, s in u] for u in want3]
    other = model.clone()
    assert other.beam_search(feats, flens, beam_size=5) == (toks, scores)


def test_a_bf16_handle_searches_in_fp32(gold, model):
    """The search stays fp32 whatever the handle's precision: on a caller's encoder output a
    bf16 handle returns the bits of the fp32 handle."""
    from wenet_amd.transducer import prefix_beam_search
    _, enc, lens = gold
    want = prefix_beam_search(model, enc, lens, 5, 0.3, 0.7)
    other = model.clone().set_compute_dtype('bf16')
    assert prefix_beam_search(other, enc, lens, 5, 0.3, 0.7) == want
    from wenet_amd import synthetic as S
    feats, flens = S.make_features(gold[0]['batch'], tuple(gold[0]['frames']), seed=gold[0]['fseed'])
    toks, scores = other.beam_search(feats.cuda(), flens, beam_size=3)
    assert len(toks) == len(scores) == gold[0]['batch'] and all(math.isfinite(s) for s in scores)


def test_a_model_without_transducer_weights_is_refused():
    from gpu_util import cached_model
    Lm, L = _lib()
    _, _, asr = cached_model('tiny_causal', 0)
    feats = torch.zeros(1, 40, 80, device='cuda')
    asr._forward_encoder(feats, torch.tensor([40]))
    n = np.zeros((1, ), dtype=np.int32)
    ln = np.zeros((1, 2), dtype=np.int32)
    tok = np.zeros((1, 2, 16), dtype=np.int32)
    sc = np.zeros((1, 2), dtype=np.float64)
    st = L.wn_transducer_beam_search(asr._h, 2, 0.3, 0.7, Lm.i32p(n), Lm.i32p(ln), Lm.i32p(tok),
                                     Lm.f64p(sc), 16, _stream())
    assert st == -1
    assert b'no transducer weights' in L.wn_last_error()
    assert b'wn_model_create_transducer' in L.wn_last_error()
