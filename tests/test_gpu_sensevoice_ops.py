"""Operator test of the SenseVoice front end (csrc/sensevoice.hip) through the hook
wn_op_sv_front, against the plain fp64 restatement tests/sensevoice_refs.ref_sv_front (checked on
the CPU in tests/test_sensevoice_host.py).

Bound on the normalised rows: 8 e_plain + 16 fp32 ulps of their scale, e_plain = the same formula
in fp32 (kernel_refs.bound).  B = 3, lengths 1 / 7 / 40 (5, 6 and 11 rows: one block of four
waves, two, three), with and without CMVN.  The batch tensor holds +-1e18 behind every
utterance's last frame, so a frame index that leaves the utterance shows; the output buffer holds
a bit pattern wherever no utterance owns.
"""
import numpy as np
import pytest
import torch

import kernel_refs as KR
import paraformer_refs as PR
import sensevoice_refs as SR

pytestmark = pytest.mark.gpu

PATTERN = 0x7fc0dead
F, M, STEP, D, LD = 80, 7, 6, 560, 576
LENS = (1, 7, 40)


def _L():
    from wenet_amd import _lib
    return _lib, _lib.lib()


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_front(c, order, lens=None, qid=None, ldo=LD):
    """The utterances as rows `order` of a (B, T, F) batch padded with +-1e18, output rows packed
    in that order with a gap of 2 behind a lead row.  Returns (rows by utterance as int32 bit
    patterns, the whole buffer, the ownership mask)."""
    _lib, L = _L()
    lens = list(c['lens']) if lens is None else list(lens)
    qid = c['qid'] if qid is None else qid
    B, T = len(lens), max(max(lens), 1) + 2
    sign = torch.where(torch.arange(F) % 2 == 0, 1.0, -1.0) * PR.POISON
    feats = sign.repeat(B, T, 1)
    s_lens, s_off, s_qid, at = [], [], [], 1
    for slot, u in enumerate(order):
        n = lens[u]
        feats[slot, :n] = c['feats'][u, :n]
        s_lens.append(n)
        s_off.append(at)
        s_qid.append(qid[u])
        at += SR.enc_rows(n) + 2
    out = torch.full((at, ldo), PATTERN, dtype=torch.int32).cuda()
    out_len = np.full(B, -7, dtype=np.int32)
    dev = {k: c[k].cuda() for k in ('embed', 'pe', 'ln_w', 'ln_b')}
    mean = c['mean'].cuda() if c['mean'] is not None else None
    istd = c['istd'].cuda() if c['istd'] is not None else None
    fd = feats.contiguous().cuda()
    _lib.check(L.wn_op_sv_front(
        fd.data_ptr(), mean.data_ptr() if mean is not None else None,
        istd.data_ptr() if istd is not None else None, dev['embed'].data_ptr(),
        dev['pe'].data_ptr(), dev['pe'].shape[0], dev['ln_w'].data_ptr(), dev['ln_b'].data_ptr(),
        out.data_ptr(), ldo, at, _lib.i32p(_i32(s_lens)), _lib.i32p(_i32(s_off)),
        _lib.i32p(_i32(s_qid)), _lib.i32p(out_len), B, T, F, M, STEP, c['xscale'], c['eps'],
        _stream()), 'sv_front')
    torch.cuda.synchronize()
    oc = out.cpu()
    own = torch.zeros(at, ldo, dtype=torch.bool)
    res = {}
    for slot, u in enumerate(order):
        rows = SR.enc_rows(lens[u])
        assert out_len[slot] == rows
        own[s_off[slot]:s_off[slot] + rows] = True
        res[u] = oc[s_off[slot]:s_off[slot] + rows]
    assert bool((oc[~own] == PATTERN).all()), 'sv_front: a store outside the owned rows'
    return res, oc, own


@pytest.mark.parametrize('cmvn', [True, False])
def test_sv_front(cmvn):
    c = SR.make_front_case(LENS, seed=5, cmvn=cmvn)
    refs = SR.front_refs(c)
    a, _, _ = run_front(c, [0, 1, 2])
    b, _, _ = run_front(c, [2, 1, 0])
    for u, n in enumerate(LENS):
        ref, plain = refs[u]
        out = a[u].view(torch.float32)
        assert out.shape == (SR.enc_rows(n), LD)
        assert bool((a[u][:, D:] == 0).all()), 'columns 560..575 must be exact zeros'
        err = (out[:, :D].double() - ref).abs().max().item()
        e_plain, scale = (plain - ref).abs().max().item(), ref.abs().max().item()
        bound = KR.bound(e_plain, scale)
        print(f'sv_front[n={n} cmvn={cmvn}] err={err:.3e} e_plain={e_plain:.3e} '
              f'scale={scale:.3e} bound={bound:.3e}')
        assert KR.cap_ok(e_plain, scale) and err <= bound
        # the query rows alone and the LFR rows alone, to the same bound
        assert (out[:4, :D].double() - ref[:4]).abs().max().item() <= bound
        assert (out[4:, :D].double() - ref[4:]).abs().max().item() <= bound
        assert torch.equal(a[u], b[u]), f'sv_front: utterance of {n} frames depends on its slot'


def test_query_rows_take_no_cmvn_and_no_frames():
    """Rows 0..3 are the table's rows, position and norm only: the same bits with and without
    CMVN and whatever the frames are; rows 4.. do not depend on the ids."""
    c = SR.make_front_case(LENS, seed=6, cmvn=True)
    a, _, _ = run_front(c, [0, 1, 2])
    n = dict(c, mean=None, istd=None)
    b, _, _ = run_front(n, [0, 1, 2])
    other = dict(c, feats=c['feats'] * 0.5 + 1.0)
    d, _, _ = run_front(other, [0, 1, 2])
    ids = dict(c, qid=[[(v + 3) % SR.N_EMBED for v in q] for q in c['qid']])
    e, _, _ = run_front(ids, [0, 1, 2])
    for u in range(len(LENS)):
        assert torch.equal(a[u][:4], b[u][:4]) and torch.equal(a[u][:4], d[u][:4])
        assert not torch.equal(a[u][4:], b[u][4:]) and not torch.equal(a[u][4:], d[u][4:])
        assert torch.equal(a[u][4:], e[u][4:]) and not torch.equal(a[u][:4], e[u][:4])
    # the same id in two places of one utterance: rows that differ by the position term only
    same = dict(c, qid=[[9, 9, 9, 9]] * 3)
    s, _, _ = run_front(same, [0, 1, 2])
    refs = SR.front_refs(same)
    for u in range(len(LENS)):
        got = s[u].view(torch.float32)[:4, :D].double()
        assert not torch.equal(got[0], got[1])
        assert (got - refs[u][0][:4]).abs().max().item() <= \
            KR.bound((refs[u][1] - refs[u][0]).abs().max().item(), refs[u][0].abs().max().item())


def test_zero_length_utterance_writes_nothing():
    c = SR.make_front_case(LENS, seed=7)
    full, _, _ = run_front(c, [0, 1, 2])
    lens = [LENS[0], 0, LENS[2]]
    got, oc, own = run_front(c, [0, 1, 2], lens=lens)
    assert got[1].shape[0] == 0
    assert torch.equal(got[0], full[0]) and torch.equal(got[2], full[2])
    assert int(own[:, 0].sum()) == SR.enc_rows(LENS[0]) + SR.enc_rows(LENS[2])


def test_narrow_pitch_has_no_pad_columns():
    """ldo = 560: nothing is written behind column 559 (the next row starts there)."""
    c = SR.make_front_case(LENS, seed=8)
    wide, _, _ = run_front(c, [0, 1, 2])
    narrow, _, _ = run_front(c, [0, 1, 2], ldo=D)
    for u in range(len(LENS)):
        assert torch.equal(narrow[u], wide[u][:, :D])


def test_refusals_before_launch():
    c = SR.make_front_case(LENS, seed=9)
    for bad in (16, -1, 1 << 20):
        qid = [list(q) for q in c['qid']]
        qid[1][2] = bad
        with pytest.raises(RuntimeError, match=r'outside \[0, 16\)'):
            run_front(c, [0, 1, 2], qid=qid)
    short = dict(c, pe=c['pe'][:8])
    with pytest.raises(RuntimeError, match='position rows'):
        run_front(short, [0, 1, 2])
    with pytest.raises(RuntimeError, match='576'):
        run_front(c, [0, 1, 2], ldo=D - 4)
    _lib, L = _L()
    dev = {k: c[k].cuda() for k in ('embed', 'pe', 'ln_w', 'ln_b')}
    out = torch.zeros(64, LD).cuda()
    fd = c['feats'].contiguous().cuda()
    out_len = np.zeros(3, dtype=np.int32)

    def call(off, lens=LENS):
        return L.wn_op_sv_front(
            fd.data_ptr(), None, None, dev['embed'].data_ptr(), dev['pe'].data_ptr(),
            dev['pe'].shape[0], dev['ln_w'].data_ptr(), dev['ln_b'].data_ptr(), out.data_ptr(), LD,
            64, _lib.i32p(_i32(lens)), _lib.i32p(_i32(off)), _lib.i32p(_i32(c['qid'])),
            _lib.i32p(out_len), 3, c['T'], F, M, STEP, c['xscale'], c['eps'], _stream())

    assert call([0, 5, 11]) == 0
    torch.cuda.synchronize()
    for off in ([0, 4, 11], [0, 5, 54], [11, 5, 0], [-1, 5, 11]):
        with pytest.raises(RuntimeError, match='outside the buffer, unordered or overlapping'):
            _lib.check(call(off), 'sv_front')
    for lens in ([1, 7, c['T'] + 1], [1, -1, 40]):
        with pytest.raises(RuntimeError, match='a length outside'):
            _lib.check(call([0, 5, 11], lens), 'sv_front')
