"""The streaming recognizer on the GPU: the resumable prefix beam search (wn_stream_*)
against the oracle's Python search on EVERY prefix and, bit for bit, against the one-shot
kernel at the end; session isolation, slot reuse, limits, endpoint counters; and
StreamingRecognizer end to end against the committed outputs of the reference's cache-based
streaming path (tests/golden/stream_*.npz)."""
import functools

import numpy as np
import pytest
import torch

from golden_util import load_case, stream_case_names

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _oracle():
    from oracle import wenet_oracle as O
    return O


# ---------------------------------------------------------------------------
# inputs: the tensors of test_search_free_functions_bit_exact and of
# test_prefix_beam_small_vocab_stress (tests/test_gpu_parity.py), built the same way
FREE = [(67, 40, 5, 4), (4233, 120, 3, 10), (5002, 64, 2, 16)]          # V, T, B, beam
STRESS = [(4, 50, 3), (5, 80, 4), (7, 60, 6), (3, 40, 2), (6, 120, 5), (8, 33, 8)]  # V, T, beam
STRESS_B = 16    # sessions per stress shape (every prefix of every session goes through the
                 # Python oracle: T^2 / 2 frames each)
CASES = [('free',) + c for c in FREE] + [('stress', V, T, STRESS_B, beam) for V, T, beam in STRESS]
CASE_IDS = ['%s-V%d-T%d-B%d-beam%d' % c for c in CASES]
SCHEDULES = ['c1', 'c4', 'c16', 'c33', 'irregular']


@functools.lru_cache(maxsize=None)
def _inputs(case):
    kind, V, T, B, beam = case
    if kind == 'free':
        g = torch.Generator().manual_seed(V + T)
        logits = torch.randn(B, T, V, generator=g) * 3.0
        logits[..., 0] += 6.0  # blank-heavy like a real CTC model
        for t in range(1, T, 3):   # repeated frames: the "repeat" / "merge" branches
            logits[:, t] = logits[:, t - 1] + 0.05 * torch.randn(B, V, generator=g)
        logp = logits.log_softmax(-1)
        lens = torch.randint(max(1, T // 2), T + 1, (B, ), generator=g)
        lens[0] = T
    else:
        g = torch.Generator().manual_seed(V * 1000 + T + beam)
        logits = torch.randn(B, T, V, generator=g) * 2
        logits[..., 0] += torch.rand(B, 1, generator=g) * 3
        for t in range(1, T, 2):
            logits[:, t] = logits[:, t - 1] + 0.1 * torch.randn(B, V, generator=g)
        logp = logits.log_softmax(-1)
        lens = torch.randint(1, T + 1, (B, ), generator=g)
        lens[0] = T
    return logp, [int(x) for x in lens]


@functools.lru_cache(maxsize=None)
def _oracle_prefix(case, b, t):
    """oracle.ctc_prefix_beam_search on the first t frames of session b."""
    logp, _ = _inputs(case)
    return _oracle().ctc_prefix_beam_search(logp[b:b + 1, :t], torch.tensor([t]), case[4])[0]


def _steps(case, schedule):
    """[(sessions, n_t)] until every session has consumed its lens[b] frames."""
    _, lens = _inputs(case)
    B = len(lens)
    done = [0] * B
    rng = np.random.RandomState(len(lens) * 131 + lens[0])
    out = []
    while any(d < n for d, n in zip(done, lens)):
        if schedule == 'irregular':
            # a random subset of the sessions, in random order, each with its own n_t (0 too)
            ss = [int(b) for b in rng.permutation(B)[:rng.randint(1, B + 1)]]
            nt = [int(min(rng.choice([0, 0, 1, 2, 3, 7, 16, 31, 32, 33, 40]), lens[b] - done[b]))
                  for b in ss]
        else:
            c = int(schedule[1:])
            ss = list(range(B))
            nt = [min(c, lens[b] - done[b]) for b in ss]
        for b, k in zip(ss, nt):
            done[b] += k
        out.append((ss, nt))
    return out


def _search(n_slots, beam, max_frames):
    from wenet_amd import search as S
    from wenet_amd.streaming import StreamSearch
    dev = torch.device(DEV)
    return StreamSearch(S._Workspace.handle(dev), dev, n_slots, beam, max_frames)


def _chunk(logp_dev, sessions, start, nt):
    """(n, Tp, V): the next nt[i] rows of each session, padded to one length."""
    Tp = max(max(nt), 1)
    x = torch.zeros((len(sessions), Tp, logp_dev.size(2)), dtype=torch.float32, device=DEV)
    for i, (b, k) in enumerate(zip(sessions, nt)):
        if k:
            x[i, :k] = logp_dev[b, start[b]:start[b] + k]
    return x


def _raw_rows(raw, i):
    """Everything wn_stream_advance wrote for row i of a call: the defined part of the arrays."""
    n = int(raw['n_hyps'][i])
    rows = []
    for j in range(raw['hyp_lens'].shape[1]):
        nl, ntl = int(raw['hyp_lens'][i, j]), int(raw['hyp_tlens'][i, j])
        rows.append((nl, ntl, raw['hyp_tokens'][i, j, :nl].tobytes(),
                     raw['hyp_times'][i, j, :ntl].tobytes(),
                     raw['hyp_scores'][i, j].tobytes(), raw['hyp_viterbi'][i, j].tobytes()))
    return (n, tuple(rows), int(raw['frames_decoded'][i]), int(raw['trailing_blank'][i]))


@functools.lru_cache(maxsize=None)
def _run(case, schedule, weak_hash=0):
    """Feed the case's tensor through B sessions on the schedule.  Records, per advance and
    session: (b, frames so far, nbest flag, DecodeResult); after the last chunk one n_t = 0
    advance of all sessions with the n-best -> the final arrays."""
    from wenet_amd import _lib
    logp, lens = _inputs(case)
    B, beam = len(lens), case[4]
    logp_dev = logp.to(DEV)
    L = _lib.lib()
    records = []
    try:
        _lib.check(L.wn_tune_set(b'beam_weak_hash', weak_hash), 'tune')
        ss = _search(B, beam, max(lens))
        done = [0] * B
        for step, (sessions, nt) in enumerate(_steps(case, schedule)):
            nbest = step % 2 == 1
            res = ss.advance(sessions, _chunk(logp_dev, sessions, done, nt), nt, nbest=nbest)
            for i, (b, k) in enumerate(zip(sessions, nt)):
                done[b] += k
                records.append((b, done[b], nbest, k, res[i], _raw_rows(res.raw, i)))
        assert done == lens
        final = ss.advance(list(range(B)), torch.zeros((B, 1, logp.size(2)), device=DEV),
                           [0] * B, nbest=True)
        ss.close()
    finally:
        L.wn_tune_set(b'beam_weak_hash', 0)
    return records, final


def _assert_matches_oracle(case, b, t, nbest, got):
    if t == 0:
        # nothing consumed: the root prefix (search.py:144-150)
        assert list(got.tokens) == [] and got.score == 0.0 and got.times == []
        return
    ref = _oracle_prefix(case, b, t)
    assert list(got.tokens) == list(ref.nbest[0]), (b, t)
    assert list(got.times) == list(ref.nbest_times[0]), (b, t)
    np.testing.assert_allclose(got.score, ref.nbest_scores[0], rtol=0, atol=1e-9)
    if nbest:
        assert [list(x) for x in got.nbest] == [list(x) for x in ref.nbest], (b, t)
        assert [list(x) for x in got.nbest_times] == [list(x) for x in ref.nbest_times], (b, t)
        np.testing.assert_allclose(got.nbest_scores, ref.nbest_scores, rtol=0, atol=1e-9)
    else:
        assert len(got.nbest) == 1      # only the 1-best is walked out


# ---------------------------------------------------------------------------
@pytest.mark.parametrize('schedule', SCHEDULES)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_stream_search_equals_oracle_on_every_prefix(case, schedule):
    """After EVERY advance each session's partial result is the oracle's Python search
    (pinned to the reference's by tests/test_oracle.py) on the frames that session has
    consumed: 1-best tokens, times, score always; the whole n-best list -- token lists,
    order, time stamps identical, scores atol 1e-9 -- on the calls that ask for it (every
    second one and the last).  No hypothesis is left out."""
    records, final = _run(case, schedule)
    _, lens = _inputs(case)
    assert len(records) >= len(lens)
    for b, t, nbest, _k, got, _raw in records:
        _assert_matches_oracle(case, b, t, nbest, got)
    for b, n in enumerate(lens):
        _assert_matches_oracle(case, b, n, True, final[b])


@pytest.mark.parametrize('schedule', SCHEDULES)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_stream_final_result_is_the_one_shot_result_bitwise(case, schedule):
    """After the last chunk every output array equals, bit for bit, what the one-shot kernel
    (search.ctc_prefix_beam_search's wn_ctc_prefix_beam_search) gives on the whole tensor:
    counts, lengths and fp64 scores as arrays, of each token / time row the first
    hyp_lens / hyp_tlens entries."""
    from wenet_amd import search as S
    logp, lens = _inputs(case)
    B, beam = len(lens), case[4]
    h, _, T, _keep = S._set_probs(logp.to(DEV), torch.tensor(lens), beam)
    _, one = S._prefix_beam(h, B, T, beam, 0, torch.device(DEV))
    _, final = _run(case, schedule)
    raw = final.raw
    for k in ('n_hyps', 'hyp_lens', 'hyp_tlens'):
        assert np.array_equal(raw[k], one[k]), k
    assert raw['hyp_scores'].tobytes() == one['hyp_scores'].tobytes()
    for b in range(B):
        for j in range(beam):
            nl, ntl = one['hyp_lens'][b, j], one['hyp_tlens'][b, j]
            assert np.array_equal(raw['hyp_tokens'][b, j, :nl], one['hyp_tokens'][b, j, :nl])
            assert np.array_equal(raw['hyp_times'][b, j, :ntl], one['hyp_times'][b, j, :ntl])


@pytest.mark.parametrize('schedule', ['c1', 'c33', 'irregular'])
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_stream_endpoint_counters(case, schedule):
    """frames_decoded / trailing_blank after every advance = a numpy evaluation of
    exp(logp[..., blank]) > 0.8 over the frames consumed so far (ctc_endpoint.cc:48-60)."""
    records, final = _run(case, schedule)
    logp, lens = _inputs(case)
    blank = np.exp(logp[..., 0].numpy().astype(np.float32)) > np.float32(0.8)

    def trailing(b, t):
        n = 0
        while n < t and blank[b, t - 1 - n]:
            n += 1
        return n
    seen_reset = False
    for b, t, _nbest, _k, got, _raw in records:
        assert got.frames_decoded == t
        assert got.trailing_blank == trailing(b, t), (b, t)
        seen_reset |= got.trailing_blank < t
    assert seen_reset or case[0] == 'free'
    for b, n in enumerate(lens):
        assert (final[b].frames_decoded, final[b].trailing_blank) == (n, trailing(b, n))


@pytest.mark.parametrize('case', [c for c in CASES if c[0] == 'stress'],
                         ids=[i for c, i in zip(CASES, CASE_IDS) if c[0] == 'stress'])
def test_stream_prefix_identity_across_launches_behind_a_2_bit_hash(case):
    """wn_tune_set("beam_weak_hash", 1): nearly every pair of prefixes passes the hash filter,
    so the result is right only if the exact sequence walk is -- here through node pools that
    were written by EARLIER launches (chunks of 4 frames, and one frame per launch)."""
    for schedule in ('c4', 'c1'):
        records, final = _run(case, schedule, 1)
        _, lens = _inputs(case)
        for b, t, nbest, _k, got, _raw in records:
            _assert_matches_oracle(case, b, t, nbest, got)
        for b, n in enumerate(lens):
            _assert_matches_oracle(case, b, n, True, final[b])


def test_stream_zero_frame_step_changes_nothing():
    """An n_t = 0 advance returns the result of the advance before it, bit for bit (1-best
    calls compared with 1-best calls), and the sessions go on as if it had not happened:
    the irregular schedule is full of such steps and still ends on the one-shot bits."""
    case = CASES[0]
    records, final = _run(case, 'irregular')
    last = {}
    zero_steps = 0
    for b, t, nbest, k, _got, raw in records:
        if k == 0 and (b, nbest) in last and last[(b, nbest)][0] == t:
            assert raw == last[(b, nbest)][1], (b, t)
            zero_steps += 1
        last[(b, nbest)] = (t, raw)
    assert zero_steps > 0
    # the final n_t = 0 n-best advance twice in a row
    logp, lens = _inputs(case)
    ss = _search(1, case[4], 64)
    x = logp[:1, :lens[0]].to(DEV)
    ss.advance([0], x, [lens[0]], nbest=True)
    z = torch.zeros((1, 1, logp.size(2)), device=DEV)
    a = ss.advance([0], z, [0], nbest=True)
    b = ss.advance([0], z, [0], nbest=True)
    assert _raw_rows(a.raw, 0) == _raw_rows(b.raw, 0)
    ss.close()


def test_stream_sessions_are_isolated_and_slots_reusable():
    """16 sessions advanced together give, session by session, the bits each gives alone; a
    slot that was reset and reused gives the bits of a fresh slot."""
    V, T, beam, B = 6, 90, 5, 16
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(B, T, V, generator=g) * 2
    logits[..., 0] += torch.rand(B, 1, generator=g) * 3
    logp = logits.log_softmax(-1).to(DEV)
    lens = [int(x) for x in torch.randint(T // 3, T + 1, (B, ), generator=g)]
    rng = np.random.RandomState(5)
    together = _search(B, beam, T)
    done = [0] * B
    while any(d < n for d, n in zip(done, lens)):
        ss = [int(b) for b in rng.permutation(B)[:rng.randint(1, B + 1)]]
        nt = [int(min(rng.choice([0, 1, 5, 16, 33]), lens[b] - done[b])) for b in ss]
        together.advance(ss, _chunk(logp, ss, done, nt), nt)
        for b, k in zip(ss, nt):
            done[b] += k
    z = torch.zeros((B, 1, V), device=DEV)
    fin = together.advance(list(range(B)), z, [0] * B, nbest=True)
    # alone, in a fresh one-slot set
    fresh = []
    for b in range(B):
        one = _search(1, beam, T)
        r = one.advance([0], logp[b:b + 1, :lens[b]].contiguous(), [lens[b]], nbest=True)
        fresh.append(_raw_rows(r.raw, 0))
        one.close()
        assert _raw_rows(fin.raw, b) == fresh[b], b
    # reuse: slot 3 of the used set, reset, fed session b's frames in other pieces
    for b in (0, 7, 15):
        together.reset([3])
        for s in range(0, lens[b], 11):
            k = min(11, lens[b] - s)
            r = together.advance([3], logp[b:b + 1, s:s + k].contiguous(), [k], nbest=True)
        assert _raw_rows(r.raw, 0) == fresh[b], b
    together.close()


def test_stream_limits():
    """Past max_frames: a non-zero status naming the limit, every session intact (the next,
    smaller advance matches the oracle); beam 17 and a handle with a context graph are
    refused with a message."""
    from wenet_amd import _lib, search as S
    from wenet_amd import context_graph as cg
    from wenet_amd.context_graph import ContextGraph
    case = ('free', 67, 40, 5, 4)
    logp, _ = _inputs(case)
    x = logp.to(DEV)
    ss = _search(2, 4, 20)
    ss.advance([0, 1], x[:2, :16].contiguous(), [16, 10])
    with pytest.raises(RuntimeError, match='max_frames = 20'):
        ss.advance([1, 0], x[:2, 16:24].contiguous(), [8, 8])     # slot 0 would reach 24
    assert ss.frames == [16, 10]
    r = ss.advance([0, 1], x[:2, 16:24][[0, 1]].contiguous(), [4, 0], nbest=True)
    _assert_matches_oracle(case, 0, 20, True, r[0])
    r = ss.advance([1], x[1:2, 10:20].contiguous(), [10], nbest=True)
    _assert_matches_oracle(case, 1, 20, True, r[0])
    with pytest.raises(RuntimeError, match='max_frames'):
        ss.advance([1], x[1:2, 20:21].contiguous(), [1])
    with pytest.raises(RuntimeError, match='twice'):
        ss.advance([1, 1], x[:2, :1].contiguous(), [0, 0])
    ss.close()
    with pytest.raises(RuntimeError, match=r'beam sizes 1\.\.16'):
        _search(1, 17, 20)
    dev = torch.device(DEV)
    h = S._Workspace.handle(dev)
    sp = torch.cuda.current_stream(dev).cuda_stream
    ok = _search(1, 4, 20)
    cg.install(_lib.lib(), h, ContextGraph(context_list=[[1, 2], [3]], context_score=2.0), sp)
    try:
        with pytest.raises(RuntimeError, match='context'):
            _search(1, 4, 20)
        with pytest.raises(RuntimeError, match='context'):
            ok.advance([0], x[:1, :4].contiguous(), [4])
    finally:
        cg.install(_lib.lib(), h, None, sp)
    r = ok.advance([0], x[:1, :4].contiguous(), [4], nbest=True)
    _assert_matches_oracle(case, 0, 4, True, r[0])
    ok.close()


# ---------------------------------------------------------------------------
# StreamingRecognizer end to end
def _pieces(n, seed, biggest):
    rng = np.random.RandomState(seed)
    cuts, at = [], 0
    while at < n:
        k = int(min(rng.randint(0, biggest + 1), n - at))
        cuts.append((at, at + k))
        at += k
    return cuts


def _check_against_golden(name, meta, arrays, rec, sid):
    from gpu_util import nbest_check
    pre = rec.finish(sid, rescoring=False)
    enc = rec.encoder_out(sid)[0].cpu().numpy()
    assert enc.shape == arrays['enc_out'].shape, (name, enc.shape)
    assert np.abs(enc - arrays['enc_out']).max() < 2e-3, name
    g = meta['prefix']
    n_ref, compared = nbest_check(pre, g['nbest'], g['nbest_scores'], g['nbest_times'], what=name)
    # at most ONE reference hypothesis left out, and only the reference's last
    assert n_ref - compared <= 1, (name, n_ref, compared)
    if n_ref - compared == 1:
        assert list(g['nbest'][-1]) not in [list(x) for x in pre.nbest], name
        assert all(list(h) in [list(x) for x in pre.nbest] for h in g['nbest'][:-1]), name
    assert list(pre.tokens) == list(g['nbest'][0]), name
    r = rec.finish(sid, rescoring=True, ctc_weight=meta['ctc_weight'],
                   reverse_weight=meta['reverse_weight'])
    gs = sorted(r.all_scores, reverse=True)
    if len(gs) < 2 or gs[0] - gs[1] > 2e-3:
        assert list(r.tokens) == meta['rescoring']['tokens'], name
    if list(r.tokens) == meta['rescoring']['tokens']:
        assert abs(r.score - meta['rescoring']['score']) < 1e-3, name


@pytest.mark.parametrize('name', stream_case_names())
def test_recognizer_single_session_vs_reference_cache_path(name):
    """One session fed the case's features in seeded random pieces: the concatenated encoder
    output, the final n-best and the rescored result against the committed outputs of the
    reference's forward_chunk_by_chunk + searches; every partial is a prefix-consistent
    result with counters that add up."""
    from gpu_util import cached_model
    from wenet_amd import synthetic as S
    from wenet_amd.streaming import StreamingRecognizer
    meta, arrays = load_case(name)
    _, _, model = cached_model(meta['config'], meta['wseed'])
    feats, _ = S.make_features(1, (meta['frames'], meta['frames']), seed=meta['fseed'])
    feats = feats[0].to(DEV)
    rec = StreamingRecognizer(model, 1, meta['chunk'], meta['left'], beam_size=meta['beam'],
                              max_seconds=meta['frames'] / 100.0)
    sid = rec.open()
    n_partials, frames = 0, 0
    for a, b in _pieces(feats.size(0), meta['fseed'], 3 * 4 * meta['chunk']):
        rec.accept(sid, feats[a:b])
        while True:
            out = rec.step()
            if not out:
                break
            r = out[sid]
            n_partials += 1
            frames += meta['chunk']
            assert r.frames_decoded == frames and 0 <= r.trailing_blank <= frames
            assert r.is_endpoint in (None, 'rule1', 'rule2', 'rule3')
            assert len(r.times) in (0, len(r.tokens))
    assert n_partials >= arrays['enc_out'].shape[0] // meta['chunk'] - 1
    _check_against_golden(name, meta, arrays, rec, sid)
    rec.close(sid)


def test_recognizer_concurrent_sessions_vs_reference_cache_path():
    """The same cases as concurrent sessions: cases that share a model AND a chunk setting
    share one recognizer (a recognizer has one decoding_chunk_size, the encoder call wants one
    window length); every recognizer also carries two more sessions with other utterances,
    fed in other pieces, so that each golden session runs in batches of up to three."""
    from gpu_util import cached_model
    from wenet_amd import synthetic as S
    from wenet_amd.streaming import StreamingRecognizer
    groups = {}
    for name in stream_case_names():
        meta, arrays = load_case(name)
        key = (meta['config'], meta['wseed'], meta['chunk'], meta['left'], meta['beam'])
        groups.setdefault(key, []).append((name, meta, arrays))
    for (config, wseed, chunk, left, beam), cases in groups.items():
        _, _, model = cached_model(config, wseed)
        rec = StreamingRecognizer(model, len(cases) + 2, chunk, left, beam_size=beam,
                                  max_seconds=6.0)
        feeds = []
        for name, meta, arrays in cases:
            f, _ = S.make_features(1, (meta['frames'], meta['frames']), seed=meta['fseed'])
            feeds.append([rec.open(), f[0].to(DEV), None, (name, meta, arrays)])
        for extra, n in enumerate((97, 260)):
            f, _ = S.make_features(1, (n, n), seed=900 + extra)
            feeds.append([rec.open(), f[0].to(DEV), None, None])
        for i, fd in enumerate(feeds):
            fd[2] = _pieces(fd[1].size(0), 40 + i, (2 + i) * 4 * chunk)
        batch_sizes = []
        while any(fd[2] for fd in feeds):
            for fd in feeds:
                if fd[2]:
                    a, b = fd[2].pop(0)
                    rec.accept(fd[0], fd[1][a:b])
            out = rec.step()
            batch_sizes.append(len(out))
        while True:
            out = rec.step()
            if not out:
                break
            batch_sizes.append(len(out))
        assert max(batch_sizes) >= 2
        for sid, _f, _p, golden in feeds:
            if golden is not None:
                _check_against_golden(golden[0] + '/concurrent', golden[1], golden[2], rec, sid)
        for fd in feeds:
            rec.finish(fd[0], rescoring=False)
            rec.close(fd[0])


def test_recognizer_batch_of_sessions_equals_single_sessions():
    """16 AIShell sessions of different lengths, opened at different steps, through step():
    every final result equals that utterance's through a one-session recognizer -- token
    lists and times identical; scores within 1e-9 when the two runs' encoder rows are bitwise
    equal (what forward_encoder_chunk_batch states: row b equals forward_encoder_chunk on
    session b alone), within the goldens' n-best tolerance should they not be."""
    from gpu_util import NBEST_TOL, cached_model
    from wenet_amd import synthetic as S
    from wenet_amd.streaming import StreamingRecognizer
    _, _, model = cached_model('aishell_u2pp', 0)
    chunk, N = 16, 16
    rng = np.random.RandomState(11)
    lengths = [int(x) for x in rng.randint(60, 420, N)]
    utts = [S.make_features(1, (n, n), seed=300 + i)[0][0].to(DEV) for i, n in enumerate(lengths)]

    def alone(f):
        rec = StreamingRecognizer(model, 1, chunk, -1, beam_size=10, max_seconds=6.0)
        sid = rec.open()
        rec.accept(sid, f)
        while rec.step():
            pass
        r = rec.finish(sid, rescoring=False)
        enc = rec.encoder_out(sid)
        rec.close(sid)
        return r, enc

    rec = StreamingRecognizer(model, N, chunk, -1, beam_size=10, max_seconds=6.0)
    sids, fed, enc, res = {}, {}, {}, {}
    step = 0
    while len(res) < N:
        if step < N:                       # one more session joins at every step
            sids[step] = rec.open()
            fed[step] = 0
        for i, sid in sids.items():
            if i in res:
                continue
            k = int(rng.choice([30, 64, 100]))
            if fed[i] < lengths[i]:
                rec.accept(sid, utts[i][fed[i]:fed[i] + k])
                fed[i] = min(fed[i] + k, lengths[i])
        rec.step()
        for i, sid in sids.items():
            if i not in res and fed[i] >= lengths[i] and not rec._sessions[sid].win.ready():
                res[i] = rec.finish(sid, rescoring=False)
                enc[i] = rec.encoder_out(sid)
        step += 1
    for i in range(N):
        r1, e1 = alone(utts[i])
        r = res[i]
        assert e1.shape == enc[i].shape
        bitwise = torch.equal(e1, enc[i])
        assert (e1 - enc[i]).abs().max().item() < 2e-3
        assert [list(x) for x in r.nbest] == [list(x) for x in r1.nbest], i
        assert [list(x) for x in r.nbest_times] == [list(x) for x in r1.nbest_times], i
        np.testing.assert_allclose(r.nbest_scores, r1.nbest_scores, rtol=0,
                                   atol=1e-9 if bitwise else NBEST_TOL)
        assert list(r.tokens) == list(r1.tokens) and r.times == r1.times, i
    for sid in sids.values():
        rec.close(sid)
