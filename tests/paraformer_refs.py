"""Plain restatements of the Paraformer pieces (wenet/models/paraformer/) the HIP kernels of
csrc/attention_d128.hip and csrc/paraformer.hip compute, in fp64 (`fp32=True`: the SAME plain
formula in fp32, the yardstick e_plain of the GPU tolerances), and the packed cases the operator
tests run them on.  Written from the reference's module text, cited file:line; nothing of the
reference is imported.  No GPU in here.

  * LFR, one utterance alone                    paraformer/layers.py:24-92
  * the encoder's position term                 paraformer/embedding.py, transformer/embedding.py:150-164
  * attention without a position term, d_k 128  paraformer/attention.py (MultiHeadedAttentionSANM /
                                                 ...CrossAtt: softmax(q k^T / sqrt(d_k)) v)
  * Cif: the alpha rows, the tail, cif()        paraformer/cif.py:55-142, 250-293
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

POISON = 1e18
DK = 128


# ---------------------------------------------------------------------------------------------
# packing: utterances between rows of +-POISON, in any order


def pack_rows(rows_list, order=None, gap=2, lead=1, ld=None):
    """rows_list[u]: (n_u, D) tensor.  Returns (buffer (rows, ld) with +-POISON wherever no
    utterance owns, offsets by UTTERANCE index, total rows); `order` = packing order of the
    utterance indices (None: 0..n-1)."""
    n = len(rows_list)
    order = list(range(n)) if order is None else list(order)
    D = rows_list[0].shape[1]
    ld = D if ld is None else ld
    offs, at = [0] * n, lead
    for u in order:
        offs[u] = at
        at += rows_list[u].shape[0] + gap
    total = max(at, 1)
    sign = torch.where(torch.arange(ld) % 2 == 0, 1.0, -1.0) * POISON
    buf = sign.repeat(total, 1).to(rows_list[0].dtype)
    for u in range(n):
        buf[offs[u]:offs[u] + rows_list[u].shape[0], :D] = rows_list[u]
    return buf.contiguous(), offs, total


def sorted_layout(offs, lens):
    """(order of utterances by offset, offsets ascending, lengths in that order)."""
    idx = sorted(range(len(offs)), key=lambda u: offs[u])
    return idx, [offs[u] for u in idx], [lens[u] for u in idx]


# ---------------------------------------------------------------------------------------------
# LFR + position + LayerNorm


def lfr_rows(n, n_step=6):
    return (n + n_step - 1) // n_step


def lfr_indices(n, m=7, n_step=6):
    """(T', m) frame indices of an utterance of n frames: row t reads the frames
    n_step t - (m - 1) // 2 + f, clamped to [0, n - 1]."""
    t = np.arange(lfr_rows(n, n_step))[:, None] * n_step - (m - 1) // 2 + np.arange(m)[None, :]
    return np.clip(t, 0, n - 1)


def lfr_indices_by_padding(n, m=7, n_step=6):
    """The same through the reference's own steps on a batch of one (layers.py:40-92): (m - 1) // 2
    copies of frame 0 in front, right_padding copies of the last frame behind, unfold(m, n_step)."""
    left = (m - 1) // 2
    n_lfr = -(-n // n_step)
    prepad = n + left
    rest = prepad - n_step * (n_lfr - 1)
    right = m - rest if m >= rest else 0
    seq = [0] * left + list(range(n)) + [n - 1] * right
    t_all = len(seq)
    rows = [seq[s:s + m] for s in range(0, t_all - m + 1, n_step)]
    return np.asarray(rows[:t_all // n_step], dtype=np.int64)


def whisper_sinusoids(rows, depth):
    """transformer/embedding.py:150-164 in fp64: [sin | cos] halves over depth // 2 timescales."""
    inc = math.log(10000.0) / (depth // 2 - 1)
    inv = torch.exp(-inc * torch.arange(depth // 2, dtype=torch.float64))
    st = torch.arange(rows, dtype=torch.float64)[:, None] * inv[None, :]
    return torch.cat([torch.sin(st), torch.cos(st)], dim=1)


def ref_layernorm(x, w, b, eps, fp32=False):
    dt = torch.float32 if fp32 else torch.float64
    x, w, b = x.to(dt), w.to(dt), b.to(dt)
    D = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / D
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / D
    return (d / torch.sqrt(var + eps) * w + b).double()


def ref_lfr_front(feats, mean, istd, pe, ln_w, ln_b, xscale, eps, m=7, n_step=6, fp32=False):
    """feats (n, F) of ONE utterance -> (T', m F): stack, GlobalCMVN (x - mean) * istd, x * xscale +
    pe[t + 1] (paraformer.py:329-350: positions start at 1), LayerNorm of layer 0."""
    dt = torch.float32 if fp32 else torch.float64
    n = feats.shape[0]
    idx = torch.from_numpy(lfr_indices(n, m, n_step))
    x = feats.to(dt)[idx].reshape(idx.shape[0], -1)
    if mean is not None:
        x = (x - mean.to(dt)) * istd.to(dt)
    x = x * torch.tensor(xscale, dtype=dt) + pe.to(dt)[1:idx.shape[0] + 1]
    return ref_layernorm(x, ln_w, ln_b, eps, fp32)


# ---------------------------------------------------------------------------------------------
# attention, d_k = 128


def ref_attention_d128(q, k, v, seqs, H, scale, fp32=False):
    """q (q_rows, >= H 128), k / v (kv_rows, >= H 128); seqs = [(q_off, q_len, kv_off, kv_len)].
    Per (sequence, head): softmax((q k^T) * scale) v.  Returns (q_rows, H 128) fp64, zero in rows
    no sequence owns."""
    dt = torch.float32 if fp32 else torch.float64
    d = H * DK
    out = torch.zeros(q.shape[0], d, dtype=torch.float64)
    for (qo, ql, ko, kl) in seqs:
        if ql == 0:
            continue
        qs = q[qo:qo + ql, :d].to(dt).view(ql, H, DK).transpose(0, 1)
        ks = k[ko:ko + kl, :d].to(dt).view(kl, H, DK).transpose(0, 1)
        vs = v[ko:ko + kl, :d].to(dt).view(kl, H, DK).transpose(0, 1)
        attn = torch.softmax(torch.matmul(qs, ks.transpose(1, 2)) * scale, dim=-1)
        out[qo:qo + ql] = torch.matmul(attn, vs).transpose(0, 1).reshape(ql, d).double()
    return out


def make_attention_d128_case(H, q_lens, kv_lens=None, seed=0, order=None):
    """Self attention (kv_lens None: Q | K | V are the three column blocks of ONE buffer of 3 H 128
    columns, as the encoder's QKV projection leaves them) or cross attention (Q in a buffer of
    H 128 + 4 columns, K | V in one of 2 H 128: ldq != ldk)."""
    g = torch.Generator().manual_seed(seed)
    d = H * DK
    n = len(q_lens)
    self_attn = kv_lens is None
    if self_attn:
        rows = [torch.randn(t, 3 * d, generator=g) for t in q_lens]
        buf, offs, total = pack_rows(rows, order, gap=3, lead=2)
        c = dict(q=buf[:, :d], k=buf[:, d:2 * d], v=buf[:, 2 * d:], buf_q=buf, buf_kv=buf,
                 ldq=3 * d, ldk=3 * d, q_cols=(0, d, 2 * d), q_rows=total, kv_rows=total,
                 q_offs=offs, kv_offs=offs, kv_lens=list(q_lens))
    else:
        qr = [torch.randn(t, d, generator=g) for t in q_lens]
        kr = [torch.randn(t, 2 * d, generator=g) for t in kv_lens]
        bq, qo, qt = pack_rows(qr, order, gap=2, lead=1, ld=d + 4)
        bk, ko, kt = pack_rows(kr, order, gap=3, lead=3)
        c = dict(q=bq[:, :d], k=bk[:, :d], v=bk[:, d:], buf_q=bq, buf_kv=bk, ldq=d + 4,
                 ldk=2 * d, q_cols=(0, 0, d), q_rows=qt, kv_rows=kt, q_offs=qo, kv_offs=ko,
                 kv_lens=list(kv_lens))
    c.update(H=H, d=d, q_lens=list(q_lens), self_attn=self_attn, scale=1.0 / math.sqrt(DK),
             seqs=[(c['q_offs'][u], q_lens[u], c['kv_offs'][u], c['kv_lens'][u])
                   for u in range(n)])
    return c


def attention_d128_refs(c):
    """(fp64 reference, e_plain, scale = the largest |v| a sequence sees)."""
    ref = ref_attention_d128(c['q'], c['k'], c['v'], c['seqs'], c['H'], c['scale'])
    plain = ref_attention_d128(c['q'], c['k'], c['v'], c['seqs'], c['H'], c['scale'], fp32=True)
    vmax = max(c['v'][ko:ko + kl].abs().max().item() for (_, ql, ko, kl) in c['seqs'] if ql > 0)
    return ref, (plain - ref).abs().max().item(), vmax


# ---------------------------------------------------------------------------------------------
# CIF


def ref_cif_alpha(h, conv_w, conv_b, out_w, out_b, smooth, noise, fp32=False):
    """h (T, d) of ONE utterance; conv_w (d, d, 3) as torch.nn.Conv1d stores it, zero padding 1 + 1
    (cif.py:41-46, 64-78 with cnn_groups 1, residual false) -> alphas (T,) fp64."""
    dt = torch.float32 if fp32 else torch.float64
    x = F.pad(h.to(dt).t().unsqueeze(0), (1, 1))
    mem = F.conv1d(x, conv_w.to(dt), conv_b.to(dt))[0].t()
    o = torch.relu(mem) @ out_w.to(dt).reshape(-1) + out_b.to(dt).reshape(())
    return torch.relu(torch.sigmoid(o) * smooth - noise).double()


def conv_w_tap_major(conv_w):
    """(d_out, d_in, 3) -> [d_out][tap * d_in + c_in]: the K = 3 d weight of the conv GEMM."""
    return conv_w.permute(0, 2, 1).reshape(conv_w.shape[0], -1).contiguous()


def cif_chain(alphas, tail, dtype=np.float32):
    """The scalar chain of cif() (cif.py:250-279) on the alphas of one utterance + the tail frame
    (cif.py:110-142), every operation in `dtype`, in the reference's order.  Returns (fire frames,
    cur per frame, remainder per frame, token_num = floor(sum in fp64, index order))."""
    a = np.concatenate([np.asarray(alphas, dtype=dtype), np.asarray([tail], dtype=dtype)])
    one = dtype(1.0)
    integrate = dtype(0.0)
    fires, cur, rem = [], np.zeros_like(a), np.zeros_like(a)
    for t in range(a.shape[0]):
        completion = dtype(one - integrate)
        integrate = dtype(integrate + a[t])
        fire = integrate >= one
        if fire:
            integrate = dtype(integrate - one)
            fires.append(t)
        cur[t] = completion if fire else a[t]
        rem[t] = dtype(a[t] - cur[t])
    total = 0.0
    for x in a:
        total += float(x)
    return fires, cur, rem, int(math.floor(total))


def ref_cif_embeds(h, alphas, tail, fp32=False):
    """h (T, d), alphas (T,) -> (embeddings (n_fire, d) fp64, fire frames, token_num): cif() over
    the T + 1 frames, the last one with a zero hidden row."""
    np_dt = np.float32 if fp32 else np.float64
    fires, cur, rem, n_tok = cif_chain(np.asarray(alphas, dtype=np_dt), tail, np_dt)
    dt = torch.float32 if fp32 else torch.float64
    hh = torch.cat([h.to(dt), torch.zeros(1, h.shape[1], dtype=dt)], dim=0)
    frame = torch.zeros(h.shape[1], dtype=dt)
    out = []
    fs = set(fires)
    for t in range(hh.shape[0]):
        frame = frame + torch.tensor(cur[t], dtype=dt) * hh[t]
        if t in fs:
            out.append(frame.double())
            frame = torch.tensor(rem[t], dtype=dt) * hh[t]
    emb = torch.stack(out) if out else torch.zeros(0, h.shape[1], dtype=torch.float64)
    return emb, fires, n_tok


def fire_margin(alphas, tail):
    """The smallest distance of an integrate value from the threshold 1.0, in fp64."""
    a = np.concatenate([np.asarray(alphas, dtype=np.float64), [tail]])
    integrate, m = 0.0, 1.0
    for x in a:
        integrate += x
        m = min(m, abs(integrate - 1.0))
        if integrate >= 1.0:
            integrate -= 1.0
    return m


# ---------------------------------------------------------------------------------------------
# the whole model on ONE utterance, from a state dict


def _lin(x, sd, name, dt, bias=True):
    y = x @ sd[name + '.weight'].to(dt).t()
    return y + sd[name + '.bias'].to(dt) if bias else y


def _norm(x, sd, name, eps, dt):
    return ref_layernorm(x, sd[name + '.weight'], sd[name + '.bias'], eps,
                         fp32=dt == torch.float32).to(dt)


def _fsmn(x, w, dt):
    """x (T, d) + depthwise conv over time, zero padding (K - 1) // 2 on both sides, no bias
    (attention.py:34-47, 66-87)."""
    K = w.shape[-1]
    y = F.conv1d(F.pad(x.t().unsqueeze(0), ((K - 1) // 2, K - 1 - (K - 1) // 2)), w.to(dt),
                 groups=x.shape[1])[0].t()
    return y + x


def _mha(q, k, v, H, dt, softmax32=False):
    """softmax32: the softmax alone in fp32, as the reference's forward_attention runs it whatever
    the module's dtype (transformer/attention.py:163-171: `scores.float()`); its .double() records
    carry that rounding, the 1e-9 pins restate it."""
    dk = q.shape[1] // H
    qs = q.view(-1, H, dk).transpose(0, 1)
    ks = k.view(-1, H, dk).transpose(0, 1)
    vs = v.view(-1, H, dk).transpose(0, 1)
    sc = torch.matmul(qs, ks.transpose(1, 2)) / math.sqrt(dk)
    att = torch.softmax(sc.float(), dim=-1).to(dt) if softmax32 else torch.softmax(sc, dim=-1)
    return torch.matmul(att, vs).transpose(0, 1).reshape(q.shape[0], -1)


def ref_sanm_attention(x, sd, p, H, dt=torch.float64, softmax32=False):
    """MultiHeadedAttentionSANM.forward (attention.py:89-116) on ONE utterance x (T, in):
    linear_out(softmax(q k^T / sqrt(d_k)) v) + fsmn(v), q | k | v = linear_q_k_v(x)."""
    qkv = _lin(x.to(dt), sd, p + '.linear_q_k_v', dt)
    d = qkv.shape[1] // 3
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    return _lin(_mha(q, k, v, H, dt, softmax32), sd, p + '.linear_out', dt) + \
        _fsmn(v, sd[p + '.fsmn_block.weight'], dt)


def _dec_ffn(z, sd, p, dt):
    """PositionwiseFeedForwardDecoderSANM (layers.py:95-123): w_2 (no bias) of the LayerNorm over
    the hidden units of relu(w_1 z)."""
    h = torch.relu(_lin(z, sd, p + '.feed_forward.w_1', dt))
    return _lin(_norm(h, sd, p + '.feed_forward.norm', 1e-5, dt), sd, p + '.feed_forward.w_2', dt,
                bias=False)


def ref_sanm_decoder_layer(y, enc, sd, p, H, dt=torch.float64, softmax32=False):
    """SanmDecoderLayer.forward (layers.py:331-379) on the token rows y (L, d) of ONE utterance
    against its encoder rows enc (T, d): t = ffn(LN1(y)); y1 = y + fsmn(LN2(t)) -- the residual is
    the layer INPUT; out = y1 + linear_out(cross attention(LN3(y1), enc)).  LN1..3: eps 1e-12."""
    y, enc = y.to(dt), enc.to(dt)
    t = _dec_ffn(_norm(y, sd, p + '.norm1', 1e-12, dt), sd, p, dt)
    y = y + _fsmn(_norm(t, sd, p + '.norm2', 1e-12, dt), sd[p + '.self_attn.fsmn_block.weight'], dt)
    q = _lin(_norm(y, sd, p + '.norm3', 1e-12, dt), sd, p + '.src_attn.linear_q', dt)
    kv = _lin(enc, sd, p + '.src_attn.linear_k_v', dt)
    d = q.shape[1]
    return y + _lin(_mha(q, kv[:, :d], kv[:, d:], H, dt, softmax32), sd,
                    p + '.src_attn.linear_out', dt)


def ref_paraformer(sd, configs, feats, fp32=False):
    """Paraformer._forward_paraformer (paraformer.py:329-360) on ONE utterance of fbank frames
    (n, 80), written out: LFR, CMVN, x sqrt(d) + pe[t + 1], the SANM encoder (layers.py:144-180,
    277-284), Cif with the tail (cif.py:55-142), the SANM decoder (layers.py:331-379, 446-477),
    log_softmax.  Returns dict(enc (T', d), alphas (T',), fires, token_num, logp (token_num, V)),
    fp64 tensors; logp is None without a token."""
    dt = torch.float32 if fp32 else torch.float64
    ec, dc, pc = configs['encoder_conf'], configs['decoder_conf'], configs['predictor_conf']
    d, H = ec['output_size'], ec['attention_heads']
    idx = torch.from_numpy(lfr_indices(feats.shape[0]))
    x = feats.to(dt)[idx].reshape(idx.shape[0], -1)
    T, D0 = x.shape
    if 'encoder.global_cmvn.mean' in sd:
        x = (x - sd['encoder.global_cmvn.mean'].to(dt)) * sd['encoder.global_cmvn.istd'].to(dt)
    x = x * torch.tensor(math.sqrt(d), dtype=dt) + whisper_sinusoids(T + 1, D0)[1:].to(dt)
    for i in range(ec['num_blocks']):
        p = 'encoder.encoders0.0' if i == 0 else f'encoder.encoders.{i - 1}'
        att = ref_sanm_attention(_norm(x, sd, p + '.norm1', 1e-5, dt), sd, p + '.self_attn', H, dt)
        x = att if i == 0 else x + att
        h = torch.relu(_lin(_norm(x, sd, p + '.norm2', 1e-5, dt), sd, p + '.feed_forward.w_1', dt))
        x = x + _lin(h, sd, p + '.feed_forward.w_2', dt)
    enc = _norm(x, sd, 'encoder.after_norm', 1e-5, dt)
    alphas = ref_cif_alpha(enc, sd['predictor.predictor.cif_conv1d.weight'],
                           sd['predictor.predictor.cif_conv1d.bias'],
                           sd['predictor.predictor.cif_output.weight'],
                           sd['predictor.predictor.cif_output.bias'], 1.0, 0.0, fp32=fp32)
    # (the tail is an fp32 value even in a .double() module: tail_process_fn builds it in fp32)
    tail = float(np.float32(pc['tail_threshold']))
    emb, fires, n_tok = ref_cif_embeds(enc, alphas.numpy(), tail, fp32=fp32)
    out = dict(enc=enc.double(), alphas=alphas, fires=fires, token_num=n_tok, logp=None)
    if n_tok == 0:
        return out
    y = torch.zeros(n_tok, d, dtype=dt)
    y[:min(n_tok, emb.shape[0])] = emb[:n_tok].to(dt)

    for j in range(dc['num_blocks']):
        y = ref_sanm_decoder_layer(y, enc, sd, f'decoder.decoders.{j}', H, dt)
    y = _dec_ffn(_norm(y, sd, 'decoder.decoders3.0.norm1', 1e-5, dt), sd, 'decoder.decoders3.0', dt)
    y = _lin(_norm(y, sd, 'decoder.after_norm', 1e-5, dt), sd, 'decoder.output_layer', dt)
    out['logp'] = torch.log_softmax(y, dim=-1).double()
    return out


CIF_ALPHA_ROWS = {
    # no fire: 0.3 + 0.2 + 0.45 < 1
    'no_fire': [0.3, 0.2],
    # a fire only on the tail frame: 0.6 + 0.45 >= 1
    'tail_only': [0.35, 0.25],
    # fires on the consecutive frames 1, 2, 3, a quiet stretch, one more fire on frame 7
    'consecutive': [0.9, 0.85, 0.9, 0.95, 0.05, 0.1, 0.05, 0.3, 0.15],
}


# ---------------------------------------------------------------------------------------------
# the fixtures of tools/gen_golden_paraformer.py (tests/golden/paraformer/)

GOLDEN_LFR_N = [1, 5, 6, 7, 24, 97]
# T' = 70, 33, 32, 4, 2, 1: three key tiles, 33 / 32, a longest-in-batch with n % 6 == 0 beside
# shorter ones (the reference's batched LFR would change them), and the zero-token case
TINY_LENS = [418, 196, 190, 24, 7, 1]
TINY_ENC_SAVED = [196, 24]       # utterances whose fp64 encoder output is recorded
TINY_FSEED = 2024
CTC_BEAM = 5
MODULE_SEED = 77

BEAUTIFY_CASES = [
    ['<sos>', '你', '好', '<eos>'],
    ['你', '好', '1', '2'],
    ['hel@@', 'lo', 'world'],
    ["it's", 'a', 'te@@', 'st'],
    ['你', '好', 'hel@@', 'lo', '世', '界'],
    ['hello', '你', '好'],
    ['we@@', 'net', '很', '好', 'yes'],
    ['<blank>', 'a'],
    [],
    ['<unk>', '你'],
    ['a', '<unk>', 'b'],
    ['3', 'd', '打', '印', 'abc@@', 'def', '!'],
]


def cif_module_inputs(d=64, T=40):
    """Input rows and weights of the recorded Cif module (fp64, seeded): h (T, d), conv_w
    (d, d, 3), conv_b (d,), out_w (1, d) -- x 4, so that the alphas spread over (0, 1) -- out_b."""
    g = torch.Generator().manual_seed(MODULE_SEED)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(h=r(T, d), conv_w=r(d, d, 3) / math.sqrt(3 * d), conv_b=0.1 * r(d),
                out_w=4.0 * r(1, d) / math.sqrt(d), out_b=0.1 * r(1))


def _seeded_sd(shapes, seed):
    """fp64 tensors by name: 2-D (and conv) weights ~ N(0, 1 / fan_in), norm weights around 1,
    every other vector ~ 0.1 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in shapes.items():
        t = torch.randn(*shape, generator=g, dtype=torch.float64)
        if len(shape) >= 2:
            t = t / math.sqrt(shape[1] * (shape[2] if len(shape) == 3 else 1))
        elif name.endswith('norm.weight') or '.norm' in name and name.endswith('weight'):
            t = 1.0 + 0.1 * t
        else:
            t = 0.1 * t
        sd[name] = t
    return sd


SANM_H, SANM_D, SANM_T, SANM_K = 2, 256, 40, 11


def sanm_attention_inputs():
    """The recorded MultiHeadedAttentionSANM: 2 heads x 128, 11 taps, a 40-frame input."""
    d = SANM_D
    sd = _seeded_sd({'linear_q_k_v.weight': (3 * d, d), 'linear_q_k_v.bias': (3 * d, ),
                     'linear_out.weight': (d, d), 'linear_out.bias': (d, ),
                     'fsmn_block.weight': (d, 1, SANM_K)}, MODULE_SEED + 10)
    g = torch.Generator().manual_seed(MODULE_SEED + 11)
    return torch.randn(SANM_T, d, generator=g, dtype=torch.float64), sd


DECL_UNITS, DECL_TOKENS = 512, 9


def sanm_decoder_layer_inputs():
    """The recorded SanmDecoderLayer: d 256, 2 heads x 128, 512 units, 11 taps; 9 token rows
    against 40 encoder frames."""
    d, F = SANM_D, DECL_UNITS
    shapes = {'feed_forward.w_1.weight': (F, d), 'feed_forward.w_1.bias': (F, ),
              'feed_forward.w_2.weight': (d, F), 'feed_forward.norm.weight': (F, ),
              'feed_forward.norm.bias': (F, ), 'self_attn.fsmn_block.weight': (d, 1, SANM_K),
              'src_attn.linear_q.weight': (d, d), 'src_attn.linear_q.bias': (d, ),
              'src_attn.linear_k_v.weight': (2 * d, d), 'src_attn.linear_k_v.bias': (2 * d, ),
              'src_attn.linear_out.weight': (d, d), 'src_attn.linear_out.bias': (d, )}
    for n in ('norm1', 'norm2', 'norm3'):
        shapes[n + '.weight'] = (d, )
        shapes[n + '.bias'] = (d, )
    sd = _seeded_sd(shapes, MODULE_SEED + 20)
    g = torch.Generator().manual_seed(MODULE_SEED + 21)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return r(DECL_TOKENS, d), r(SANM_T, d), sd


def features(n, seed):
    """(n, 80) log-mel-like frames: smooth in time, mean ~11, std ~3."""
    g = torch.Generator().manual_seed(seed * 1000 + n)
    x = torch.randn(n, 80, generator=g)
    x[1:] = 0.6 * x[:-1] + 0.8 * x[1:]
    return (11.0 + 3.0 * x).contiguous()


def tiny_features():
    return [features(n, TINY_FSEED) for n in TINY_LENS]


def load_golden(directory, stem):
    """(meta dict, arrays dict) of <stem>.npz + <stem>_<i>.npz, `__part<i>` row blocks joined."""
    import json
    import os
    arrays, meta, i = {}, None, 0
    while True:
        path = os.path.join(directory, f'{stem}.npz' if i == 0 else f'{stem}_{i}.npz')
        if not os.path.exists(path):
            break
        with np.load(path) as z:
            for k in z.files:
                if k == 'meta':
                    meta = json.loads(bytes(z[k]).decode())
                else:
                    arrays[k] = z[k]
        i += 1
    parts = {}
    for k in sorted(arrays):
        if '__part' in k:
            base, idx = k.split('__part')
            parts.setdefault(base, []).append((int(idx), arrays[k]))
    for base, lst in parts.items():
        arrays[base] = np.concatenate([a for _, a in sorted(lst, key=lambda t: t[0])], axis=0)
    return meta, arrays
