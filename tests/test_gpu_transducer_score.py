"""GPU checks of the teacher-forced transducer score and of transducer + attention rescoring
(wenet_amd/csrc/transducer_score.hip, cabi_transducer_score.hip, wenet_amd/transducer.py):
 (a) wn_op_joint_logp_gather against fp64: error <= 4 x (torch's fp32 CPU log_softmax of the same
     rows against fp64) + 1e-6; the same rows at other tile offsets and in another M: same bits;
 (b) wn_op_rnnt_lattice against the fp64 restatement within 1e-12 (T + U) relative; -inf in gives
     -inf out, never NaN;
 (c) wn_transducer_score on the recorded encoder output (tests/golden/rnnt/rnnt_rescore_tiny.npz):
     within 4 e_td + 1e-6 of the fp64 reference; the same bits alone, batched, permuted;
 (d) rescoring on the fixture: every recorded run's winner and score (4 e_score + 1e-6), from the
     recorded encoder output and end to end from the features, alone and batched, both search
     types, through transducer_attention_rescoring and decode;
 (e) a vocabulary of 65 x 128 + 9 against the fp64 restatement.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import transducer_formulation as TF
import transducer_score_formulation as SF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from wenet_amd import _lib as L
    return L, L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- (a) joint + log-softmax + gather ---------------------------------------------------------
N_ENC, N_PRED = 40, 5


def _gather_case(J, V, seed):
    g = torch.Generator().manual_seed(seed)
    enc_proj = torch.randn(N_ENC, J, generator=g)
    pred_proj = torch.randn(N_PRED, J, generator=g)
    W = torch.randn(V, J, generator=g) * (3.0 / math.sqrt(J))
    bias = torch.randn(V, generator=g) * 0.1
    return enc_proj, pred_proj, W, bias


def _lists(M, V, rng):
    """Column lists of M rows: column 0, V - 1, one in the last partial 128-block, a repeated
    column, lengths 1 and 17, then random ones."""
    last = (V - 1) // 128 * 128 + (V - 1) % 128 // 2       # in the last block, not V - 1
    fixed = [[0], [V - 1, last, 0], [last] + [5, 5] + rng.integers(0, V, size=14).tolist()]
    out = []
    for m in range(M):
        out.append(fixed[m] if m < len(fixed)
                   else rng.integers(0, V, size=int(rng.integers(1, 18))).tolist())
    return out


def _gather_run(dev, row_enc, row_pred, lists, J, V):
    Lm, L = _lib()
    enc_proj, pred_proj, W, bias = dev
    M = len(row_enc)
    col_off = np.zeros(M + 1, dtype=np.int32)
    col_off[1:] = np.cumsum([len(x) for x in lists])
    cols = np.array([c for x in lists for c in x], dtype=np.int32)
    out = np.full((len(cols), ), 7.5, dtype=np.float32)
    st = L.wn_op_joint_logp_gather(enc_proj.data_ptr(), N_ENC, pred_proj.data_ptr(), N_PRED,
                                   Lm.i32p(np.ascontiguousarray(row_enc, dtype=np.int32)),
                                   Lm.i32p(np.ascontiguousarray(row_pred, dtype=np.int32)),
                                   W.data_ptr(), bias.data_ptr(), M, J, V, Lm.i32p(col_off),
                                   Lm.i32p(cols), Lm.f32p(out), _stream())
    assert st == 0, L.wn_last_error()
    return [out[col_off[m]:col_off[m + 1]] for m in range(M)]


def _logp_rows(case, row_enc, row_pred, dtype):
    enc_proj, pred_proj, W, bias = [t.to(dtype) for t in case]
    with torch.no_grad():
        lp = torch.log_softmax(torch.tanh(enc_proj[row_enc] + pred_proj[row_pred]) @ W.T + bias, dim=-1)
    return lp.double().numpy()


@pytest.mark.parametrize('M', [3, 48, 130])
@pytest.mark.parametrize('J,V', [(160, 67), (512, 4233), (32, 8329), (1024, 300)])
def test_joint_logp_gather_against_fp64(J, V, M):
    case = _gather_case(J, V, seed=J + V)
    rng = np.random.default_rng(M * 7 + J)
    row_enc = rng.integers(0, N_ENC, size=M)
    row_pred = rng.integers(0, N_PRED, size=M)
    if M > 3:
        row_enc[rng.random(M) < 0.2] = -1
        row_enc[:3], row_enc[M - 1] = [11, 3, 7], -1
    lists = _lists(M, V, rng)
    assert {len(x) for x in lists} >= {1, 17}
    live = row_enc >= 0
    dev = tuple(t.cuda().contiguous() for t in case)
    got = _gather_run(dev, row_enc, row_pred, lists, J, V)
    ref = _logp_rows(case, row_enc[live], row_pred[live], torch.float64)
    plain = _logp_rows(case, row_enc[live], row_pred[live], torch.float32)
    e_plain = np.abs(plain - ref).max()
    bar = 4 * e_plain + 1e-6
    err, r = 0.0, 0
    for m in range(M):
        if not live[m]:
            assert np.isnan(got[m]).all(), m          # inert rows: nothing written
            continue
        err = max(err, np.abs(got[m].astype(np.float64) - ref[r][lists[m]]).max())
        r += 1
    print(f'logp_gather J={J} V={V} M={M}: err {err:.3e}, torch fp32 {e_plain:.3e}, ratio '
          f'{err / e_plain:.2f}')
    assert err <= bar, (err, e_plain)
    # a repeated column: the same bits twice
    assert got[2][1].view(np.int32) == got[2][2].view(np.int32)
    # the same rows at other tile offsets (shifted by 1, 31, 33, 64 inert rows) and alone (M = 1)
    for shift in (1, 31, 33, 64):
        pad_e = np.concatenate([np.full(shift, -1), row_enc])
        pad_p = np.concatenate([np.zeros(shift, dtype=np.int64), row_pred])
        again = _gather_run(dev, pad_e, pad_p, [[0]] * shift + lists, J, V)[shift:]
        for m in np.flatnonzero(live):
            assert np.array_equal(again[m].view(np.int32), got[m].view(np.int32)), (shift, m)
    for m in np.flatnonzero(live)[[0, -1]]:
        one = _gather_run(dev, row_enc[m:m + 1], row_pred[m:m + 1], [lists[m]], J, V)[0]
        assert np.array_equal(one.view(np.int32), got[m].view(np.int32)), m


# ---- (b) the lattice ----------------------------------------------------------------------------
LATTICES = [(1, 0), (1, 3), (2, 1), (29, 0), (29, 5), (16, 63), (16, 64), (15, 70), (5, 12)]


def _lattice_run(lat):
    """lat: [(lp_blank (T, U + 1), lp_label (T, U)), ...] -> scores."""
    Lm, L = _lib()
    T = np.array([b.shape[0] for b, _ in lat], dtype=np.int32)
    U = np.array([b.shape[1] - 1 for b, _ in lat], dtype=np.int32)
    eb = np.concatenate([b.ravel() for b, _ in lat] + [np.zeros(1)]).astype(np.float32)
    el = np.concatenate([l.ravel() for _, l in lat] + [np.zeros(1)]).astype(np.float32)
    out = np.full((len(lat), ), 7.5)
    st = L.wn_op_rnnt_lattice(len(lat), Lm.i32p(T), Lm.i32p(U), Lm.f32p(eb), Lm.f32p(el),
                              Lm.f64p(out), _stream())
    assert st == 0, L.wn_last_error()
    return out


def test_lattice_against_the_restatement():
    rng = np.random.default_rng(21)
    lat, kind = [], []
    for T, U in LATTICES:
        for variant in ('plain', 'holes', 'wall'):
            lb = np.log(rng.uniform(0.05, 0.9, size=(T, U + 1))).astype(np.float32)
            ll = np.log(rng.uniform(0.05, 0.9, size=(T, U))).astype(np.float32)
            if variant == 'holes':          # -inf entries that leave some path open
                lb[rng.random(lb.shape) < 0.15] = -np.inf
                ll[rng.random(ll.shape) < 0.15] = -np.inf
                lb[T - 1, U] = np.float32(-0.5)
            if variant == 'wall':           # an all -inf column: no path at all (U > 0)
                if U == 0:
                    lb[T // 2, 0] = -np.inf
                else:
                    ll[:, U // 2] = -np.inf
            lat.append((lb, ll))
            kind.append((T, U, variant))
    got = _lattice_run(lat)
    assert not np.isnan(got).any()
    n_inf = 0
    for (T, U, variant), (lb, ll), g in zip(kind, lat, got):
        want = SF.lattice(lb, ll)
        if variant == 'wall':
            assert want == -np.inf
        if want == -np.inf:
            assert g == -np.inf, (T, U, variant, g)
            n_inf += 1
        else:
            assert abs(g - want) <= 1e-12 * (T + U) * abs(want), (T, U, variant, g, want)
    assert n_inf >= len(LATTICES)
    # each lattice alone: the same bits; T = 0 answers -inf
    for i in (0, 5, 17, 22):
        assert _lattice_run([lat[i]])[0] == got[i] or (np.isneginf(got[i]))
    assert _lattice_run([(np.zeros((0, 3)), np.zeros((0, 2)))])[0] == -np.inf


# ---- (c) the score on the recorded encoder output -----------------------------------------------
@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'rnnt', 'rnnt_rescore_tiny.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    return meta, torch.from_numpy(z['enc']).cuda(), meta['enc_lens']


@pytest.fixture(scope='module')
def model(gold):
    from wenet_amd import Transducer
    from wenet_amd import synthetic as S
    configs = S.make_configs(gold[0]['config'])
    return Transducer(configs, S.make_state_dict(configs, gold[0]['wseed']), device='cuda')


def _run_key(stype, sw, beam, wi):
    return f'{stype}_{sw[0]}_{sw[1]}_{beam}_{wi}'


def test_transducer_score_on_the_recorded_encoder_output(gold, model):
    from wenet_amd.transducer import transducer_score
    meta, enc, lens = gold
    bar = 4 * meta['e_td'] + 1e-6
    worst = 0.0
    for beam in meta['beams']:
        for stype, sw in (('transducer', (0.3, 0.7)), ('ctc', (1.0, 0.0))):
            want = meta['runs'][_run_key(stype, sw, beam, 1)]['fp64']
            hyps = [[t for t, _ in u['nbest']] for u in want]
            got = transducer_score(model, enc, lens, hyps)
            err = max(abs(a - c) for g, u in zip(got, want) for a, c in zip(g, u['td']))
            worst = max(worst, err)
            assert err <= bar, (beam, stype, err, bar)
            rows, unshared, nodes = model.last_rnnt_score_rows
            assert rows == sum(n * len(SF.build_trie(h, meta['blank'])['parent'])
                               for n, h in zip(lens, hyps))
            assert unshared == sum(n * (len(t) + 1) for n, h in zip(lens, hyps) for t in h)
            if beam >= 5:
                assert rows < unshared, (rows, unshared)
            # alone, in another order of the batch, with the hypotheses permuted: the same bits
            for b in range(len(lens)):
                assert transducer_score(model, enc[b:b + 1], lens[b:b + 1], [hyps[b]]) == [got[b]]
            order = [2, 0, 1]
            assert transducer_score(model, enc[order].contiguous(), [lens[b] for b in order],
                                    [hyps[b] for b in order]) == [got[b] for b in order]
            rev = transducer_score(model, enc, lens, [h[::-1] for h in hyps])
            assert rev == [g[::-1] for g in got]
            # fewer hypotheses in one utterance than in the others, and an utterance of no frames
            if beam >= 5:
                some = [hyps[0][:2], hyps[1], hyps[2]]
                got2 = transducer_score(model, enc, [lens[0], 0, lens[2]], some)
                assert got2[0] == got[0][:2] and got2[2] == got[2]
                assert all(v == -math.inf for v in got2[1]) and len(got2[1]) == len(hyps[1])
    print(f"transducer score: worst err {worst:.3e}, e_td {meta['e_td']:.3e}, ratio "
          f"{worst / meta['e_td']:.2f}")


def test_transducer_score_refusals(gold, model):
    from wenet_amd.transducer import transducer_score
    _, enc, lens = gold
    V = model._cfg.vocab
    ok = [[[1, 2]], [[3]], [[]]]
    assert all(math.isfinite(v) for u in transducer_score(model, enc, lens, ok) for v in u)
    with pytest.raises(RuntimeError, match='token outside'):
        transducer_score(model, enc, lens, [[[1, V]], [[3]], [[]]])
    with pytest.raises(RuntimeError, match='token outside'):
        transducer_score(model, enc, lens, [[[1, -1]], [[3]], [[]]])
    with pytest.raises(RuntimeError, match='n_hyps'):
        transducer_score(model, enc, lens, [[[1]], [], [[]]])
    with pytest.raises(RuntimeError, match='beam must be'):
        transducer_score(model, enc, lens, [[[1]] * 17, [[3]], [[]]])
    with pytest.raises(ValueError, match='n-bests'):
        transducer_score(model, enc, lens, ok[:2])
    # a label equal to the blank id is a column like any other
    assert math.isfinite(transducer_score(model, enc, lens, [[[0, 1]], [[3]], [[]]])[0][0])


def test_entries_beyond_n_hyps_are_never_read(gold, model):
    """As wn_rescore, the call reads the lengths and tokens of hypotheses k < n_hyps[b] only: a
    caller may leave anything behind them."""
    Lm, L = _lib()
    meta, enc, lens = gold
    model._set_encoder_out(enc, torch.as_tensor(lens))
    hyps = [[t for t, _ in u['nbest']]
            for u in meta['runs'][_run_key('transducer', (0.3, 0.7), 5, 1)]['fp64']]
    hyps = [hyps[0][:2], hyps[1][:5], hyps[2][:1]]
    B, beam = 3, 5
    max_len = max(len(h) for u in hyps for h in u)

    def run(fill_len, fill_tok):
        n = np.array([len(u) for u in hyps], dtype=np.int32)
        ln = np.full((B, beam), fill_len, dtype=np.int32)
        tok = np.full((B, beam, max_len), fill_tok, dtype=np.int32)
        for b, u in enumerate(hyps):
            for k, h in enumerate(u):
                ln[b, k] = len(h)
                tok[b, k, :] = fill_tok
                tok[b, k, :len(h)] = h
        td = np.full((B, beam), 7.5)
        st = L.wn_transducer_score(model._h, beam, Lm.i32p(n), Lm.i32p(ln), Lm.i32p(tok), max_len,
                                   Lm.f64p(td), _stream())
        assert st == 0, L.wn_last_error()
        return td

    want = run(0, 0)
    for fill_len, fill_tok in ((-1, -1), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31),
                               (max_len + 1, model._cfg.vocab)):
        got = run(fill_len, fill_tok)
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (fill_len, fill_tok)
    for b, u in enumerate(hyps):
        assert np.isfinite(want[b, :len(u)]).all() and np.isneginf(want[b, len(u):]).all()


def test_a_bf16_handle_scores_in_fp32(gold, model):
    from wenet_amd.transducer import transducer_score
    meta, enc, lens = gold
    hyps = [[t for t, _ in u['nbest']]
            for u in meta['runs'][_run_key('transducer', (0.3, 0.7), 5, 1)]['fp64']]
    other = model.clone().set_compute_dtype('bf16')
    assert transducer_score(other, enc, lens, hyps) == transducer_score(model, enc, lens, hyps)


def test_a_model_without_transducer_weights_is_refused():
    from gpu_util import cached_model
    Lm, L = _lib()
    _, _, asr = cached_model('tiny_causal', 0)
    asr._forward_encoder(torch.zeros(1, 40, 80, device='cuda'), torch.tensor([40]))
    n = np.ones((1, ), dtype=np.int32)
    ln = np.zeros((1, 2), dtype=np.int32)
    tok = np.zeros((1, 2, 4), dtype=np.int32)
    sc = np.zeros((1, 2), dtype=np.float64)
    st = L.wn_transducer_score(asr._h, 2, Lm.i32p(n), Lm.i32p(ln), Lm.i32p(tok), 4, Lm.f64p(sc),
                               _stream())
    assert st == -1
    assert b'no transducer weights' in L.wn_last_error()


# ---- (d) rescoring on the fixture ------------------------------------------------------------------
def _check_runs(meta, rescore, what):
    """rescore(stype, sw, beam, (cw, aw, tw, rw)) -> DecodeResults of the batch; against every
    recorded run."""
    bar = 4 * meta['e_score'] + 1e-6
    worst = 0.0
    for key, run in meta['runs'].items():
        res = rescore(run['search'], run['search_weights'], run['beam'], run['weights'])
        for b, (r, u) in enumerate(zip(res, run['fp64'])):
            assert list(r.tokens) == u['tokens'], (what, key, b)
            worst = max(worst, abs(r.score - u['score']))
            assert abs(r.score - u['score']) <= bar, (what, key, b, r.score, u['score'])
    print(f"{what}: worst score err {worst:.3e}, e_score {meta['e_score']:.3e}, ratio "
          f"{worst / meta['e_score']:.2f}")


def test_rescoring_on_the_recorded_encoder_output(gold, model):
    from wenet_amd.transducer import attention_rescoring
    meta, enc, lens = gold

    def batched(stype, sw, beam, w):
        res = attention_rescoring(model, enc, lens, beam, reverse_weight=w[3], ctc_weight=w[0],
                                  attn_weight=w[1], transducer_weight=w[2],
                                  search_ctc_weight=sw[0], search_transducer_weight=sw[1],
                                  beam_search_type=stype)
        run = meta['runs'][_run_key(stype, sw, beam, meta['rescore_weights'].index(list(w)))]
        for r, u in zip(res, run['fp64']):       # the n-best in search order, every score
            assert r.nbest == [t for t, _ in u['nbest']]
            assert max(abs(a - c) for a, c in zip(r.nbest_scores, u['final'])) \
                <= 4 * meta['e_score'] + 1e-6
            assert max(abs(a - c) for a, c in zip(r.attn_scores, u['attn'])) \
                <= 4 * meta['e_attn'] + 1e-6
        return res

    def alone(stype, sw, beam, w):
        return [attention_rescoring(model, enc[b:b + 1], lens[b:b + 1], beam, reverse_weight=w[3],
                                    ctc_weight=w[0], attn_weight=w[1], transducer_weight=w[2],
                                    search_ctc_weight=sw[0], search_transducer_weight=sw[1],
                                    beam_search_type=stype)[0] for b in range(len(lens))]

    _check_runs(meta, batched, 'recorded encoder output, batched')
    _check_runs(meta, alone, 'recorded encoder output, alone')


def test_rescoring_end_to_end(gold, model):
    from wenet_amd import synthetic as S
    from wenet_amd.search import DecodeResult
    meta, _, _ = gold
    feats, flens = S.make_features(meta['batch'], tuple(meta['frames']), seed=meta['fseed'])
    feats = feats.cuda()

    def method(stype, sw, beam, w):
        toks, scores = model.transducer_attention_rescoring(
            feats, flens, beam, reverse_weight=w[3], ctc_weight=w[0], attn_weight=w[1],
            transducer_weight=w[2], search_ctc_weight=sw[0], search_transducer_weight=sw[1],
            beam_search_type=stype)
        return [DecodeResult(t, score=s) for t, s in zip(toks, scores)]

    def method_alone(stype, sw, beam, w):
        out = []
        for b in range(meta['batch']):
            n = int(flens[b])
            toks, scores = model.transducer_attention_rescoring(
                feats[b:b + 1, :n], flens[b:b + 1], beam, reverse_weight=w[3], ctc_weight=w[0],
                attn_weight=w[1], transducer_weight=w[2], search_ctc_weight=sw[0],
                search_transducer_weight=sw[1], beam_search_type=stype)
            out.append(DecodeResult(toks[0], score=scores[0]))
        return out

    def decode(stype, sw, beam, w):
        res = model.decode(['rnnt_beam_search', 'rnnt_beam_attn_rescoring'], feats, flens,
                           beam_size=beam, ctc_weight=w[0], reverse_weight=w[3], attn_weight=w[1],
                           transducer_weight=w[2], search_ctc_weight=sw[0],
                           search_transducer_weight=sw[1], beam_search_type=stype)
        assert sorted(res) == ['rnnt_beam_attn_rescoring', 'rnnt_beam_search']
        if stype == 'transducer':          # one search serves both modes
            for r, s in zip(res['rnnt_beam_attn_rescoring'], res['rnnt_beam_search']):
                assert r.nbest == s.nbest and len(r.nbest_scores) == len(r.nbest)
        return res['rnnt_beam_attn_rescoring']

    _check_runs(meta, method, 'transducer_attention_rescoring, batched')
    _check_runs(meta, method_alone, 'transducer_attention_rescoring, alone')
    _check_runs(meta, decode, 'decode')
    # transducer_weight = 0 launches no score kernels: the statistics of the last call stay
    model.transducer_attention_rescoring(feats, flens, 5, attn_weight=0.4, ctc_weight=0.3,
                                         transducer_weight=0.3)
    stats = model.last_rnnt_score_rows
    assert stats[0] > 0
    model.last_rnnt_score_rows = None
    model.transducer_attention_rescoring(feats, flens, 5, attn_weight=0.5, ctc_weight=0.5)
    assert model.last_rnnt_score_rows is None
    rows, unshared, nodes = (np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64),
                             np.zeros(1, dtype=np.int32))
    Lm, L = _lib()
    assert L.wn_transducer_score_stats(model._h, Lm.i64p(rows), Lm.i64p(unshared),
                                       Lm.i32p(nodes)) == 0
    assert (int(rows[0]), int(unshared[0]), int(nodes[0])) == stats
    # existing modes are as before beside the new one
    both = model.decode(['rnnt_beam_attn_rescoring', 'attention_rescoring', 'rnnt_greedy_search'],
                        feats, flens, beam_size=5, ctc_weight=0.3, attn_weight=0.4,
                        transducer_weight=0.3, reverse_weight=0.3)
    only = model.decode(['attention_rescoring', 'rnnt_greedy_search'], feats, flens, beam_size=5,
                        ctc_weight=0.3, reverse_weight=0.3)
    for k in only:
        assert [(list(r.tokens), r.score) for r in both[k]] == \
            [(list(r.tokens), r.score) for r in only[k]], k
    # the CTC n-best beside the CTC modes of the same call, and beside modes that need no beam
    kw = dict(beam_size=5, ctc_weight=0.3, attn_weight=0.4, transducer_weight=0.3,
              reverse_weight=0.3, beam_search_type='ctc')
    alone = model.decode(['rnnt_beam_attn_rescoring'], feats, flens, **kw)
    modes = ['attention_rescoring', 'ctc_prefix_beam_search', 'ctc_greedy_search']
    mixed = model.decode(['rnnt_beam_attn_rescoring'] + modes, feats, flens, **kw)
    plain = model.decode(modes, feats, flens, beam_size=5, ctc_weight=0.3, reverse_weight=0.3)
    light = model.decode(['rnnt_beam_attn_rescoring', 'ctc_greedy_search', 'rnnt_greedy_search'],
                         feats, flens, **kw)
    for got in (mixed, light):
        assert [(r.tokens, r.score, r.nbest, r.nbest_scores)
                for r in got['rnnt_beam_attn_rescoring']] == \
            [(r.tokens, r.score, r.nbest, r.nbest_scores) for r in alone['rnnt_beam_attn_rescoring']]
    for k in modes:
        assert [(list(r.tokens), r.score) for r in mixed[k]] == \
            [(list(r.tokens), r.score) for r in plain[k]], k
    assert [list(r.tokens) for r in light['ctc_greedy_search']] == \
        [list(r.tokens) for r in plain['ctc_greedy_search']]
    # its n-best is the CTC prefix beam search's own
    for r, c in zip(alone['rnnt_beam_attn_rescoring'], plain['ctc_prefix_beam_search']):
        assert r.nbest == [list(t) for t in c.nbest]


# ---- (e) a vocabulary of 65 x 128 + 9 ---------------------------------------------------------------
# No recorded reference at this size: the fp64 restatement is the reference for the transducer
# score, with the bar of (a) carried through the lattice.  e_lp: the error of the gathered
# log-probs by torch in fp32 on the CPU against fp64.  log_add does not amplify the errors of its
# two arguments (its partial derivatives add up to 1), and a path adds T' + U log-probs, so
#     e_td <= (T' + U) e_lp.
# Winners are compared with transducer_weight = 1 alone (attn_weight = ctc_weight = 0): the final
# score is then the transducer score, and the test asserts on the fp64 side that the winner's gap
# exceeds twice the bar it uses.
WIDE_LENS = [21, 8, 16]
WIDE_BEAM = 4


def test_score_with_a_wide_vocabulary():
    from wenet_amd import Transducer
    from wenet_amd import synthetic as S
    from wenet_amd.transducer import attention_rescoring, prefix_beam_search, transducer_score
    configs = S.make_configs('tiny_rnnt_wide')
    sd = S.make_state_dict(configs, 3)
    d = configs['encoder_conf']['output_size']
    rng = np.random.default_rng(1234)
    enc = rng.standard_normal((len(WIDE_LENS), max(WIDE_LENS), d)).astype(np.float32)
    sdn = {k: v.numpy() for k, v in sd.items()}
    W = TF.weights64(sdn, 2)
    model = Transducer(configs, sd, device='cuda')
    tenc = torch.from_numpy(enc).cuda()
    nbest = prefix_beam_search(model, tenc, WIDE_LENS, WIDE_BEAM, 0.3, 0.7)
    hyps = [[t for t, _ in u] for u in nbest]
    assert any(t >= 128 for u in hyps for h in u for t in h)       # beyond column block 0
    got = transducer_score(model, tenc, WIDE_LENS, hyps)
    # the fp64 side, and e_lp by torch in fp32
    W32 = {k: torch.from_numpy(np.ascontiguousarray(sdn[k])) for k in
           ('joint.enc_ffn.weight', 'joint.enc_ffn.bias', 'joint.ffn_out.weight',
            'joint.ffn_out.bias')}
    worst = 0.0
    for b, n in enumerate(WIDE_LENS):
        want = SF.transducer_scores(enc[b, :n], hyps[b], W, 0)
        trie = SF.build_trie(hyps[b], 0)
        pp = SF.trie_pred_proj(trie, W)
        enc_proj = enc[b, :n].astype(np.float64) @ W['enc_ffn'][0].T + W['enc_ffn'][1]
        lp64 = SF.gathered_logp(enc_proj, pp, trie, W)
        with torch.no_grad():
            ep32 = torch.from_numpy(enc[b, :n]) @ W32['joint.enc_ffn.weight'].T + W32['joint.enc_ffn.bias']
            ent_node = np.repeat(np.arange(len(trie['parent'])), np.diff(trie['col_off']))
            lp32 = np.stack([torch.log_softmax(
                torch.tanh(ep32[t] + torch.from_numpy(pp).float()) @ W32['joint.ffn_out.weight'].T
                + W32['joint.ffn_out.bias'], dim=-1).double().numpy()[ent_node, trie['cols']]
                for t in range(n)])
        e_lp = float(np.abs(lp32 - lp64).max())
        longest = max(len(h) for h in hyps[b])
        bar = 4 * (n + longest) * e_lp + 1e-6
        err = max(abs(a - c) for a, c in zip(got[b], want))
        worst = max(worst, err / bar)
        print(f'wide score utterance {b}: err {err:.3e}, e_lp {e_lp:.3e}, bar {bar:.3e}')
        assert err <= bar, (b, err, bar)
        srt = sorted(want, reverse=True)
        assert srt[0] - srt[1] > 2 * bar, (b, srt[0] - srt[1], bar)
        res = attention_rescoring(model, tenc[b:b + 1], [n], WIDE_BEAM, transducer_weight=1.0,
                                  search_ctc_weight=0.3, search_transducer_weight=0.7)[0]
        best, _ = SF.combine([0.0] * len(want), [0.0] * len(want), want, 0.0, 0.0, 1.0)
        assert res.nbest == hyps[b] and list(res.tokens) == hyps[b][best]
        assert abs(res.score - want[best]) <= bar
