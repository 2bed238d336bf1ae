"""SenseVoice Small (`model: sensevoice_small`) on libwenet_amd's HIP kernels.

Mirrors (reference file:line):
  * SenseVoiceSmall.__init__ / decode            wenet/models/sensevoice/sensevoice_small_model.py:143-290
  * SanmEncoderWithTp                            wenet/models/sensevoice/sensevoice_small_model.py:21-140
  * LFR, AliParaformerEncoderLayer               wenet/models/paraformer/layers.py
  * the converter's train.yaml                   wenet/models/sensevoice/convert_sensevoice_small_to_wenet_config_and_ckpt.py

Four query rows (language | event | emotion | text norm, rows of a 16 x 560 embedding table) stand
in front of the LFR rows of an utterance; the SANM stack, after_norm, the tp stack and tp_norm run
over all of them and the CTC head decodes every frame, the four query frames included.  The
kernels: csrc/sensevoice.hip (the front end), csrc/cabi_sensevoice.hip (the driver), the layer
stacks are the Paraformer's.  The CTC searches are `ASRModel`'s.

Deviations from the reference:
  * every utterance is encoded as the reference encodes it ALONE (the batched LFR is batch
    dependent, as for the Paraformer);
  * an utterance without feature frames gives DecodeResult([]) (the reference raises inside LFR);
  * the caller's speech_lengths is left as it is (the reference adds 4 to it in place);
  * `infos['lid']` / `infos['itn']` may be lists with one entry per utterance.
"""
import ctypes
from typing import Dict, List

import numpy as np
import torch

from wenet_amd import _lib
from wenet_amd.model import ASRModel, _stream_ptr
from wenet_amd.search import DecodeResult

METHODS = ('ctc_greedy_search', 'ctc_prefix_beam_search')
MAX_FRAMES = 2048      # LFR frames (60 ms each) the position rows of a handle cover
LFR_M, LFR_N = 7, 6    # sensevoice_small_model.py:167: the model builds LFR() with its defaults
N_QUERY, N_EMBED = 4, 16
# sensevoice_small_model.py:173-175
LID_DICT = {'auto': 0, 'zh': 3, 'en': 4, 'yue': 7, 'ja': 11, 'ko': 12, 'nospeech': 13}
TEXTNORM_DICT = {'withitn': 14, 'woitn': 15}
EVENT_ROW, EMOTION_ROW = 1, 2


def _refuse(key, got, want):
    raise NotImplementedError(
        f'{key}={got!r} is outside the accelerated path (the SenseVoice kernels need {want!r})')


def out_len(n: int) -> int:
    """Encoder frames of an utterance of n feature frames decoded alone."""
    return -(-n // LFR_N) + N_QUERY if n > 0 else 0


def lid_row(lid) -> int:
    """sensevoice_small_model.py:273: an unknown language is `auto`."""
    return LID_DICT.get(lid, 0) if isinstance(lid, str) else 0


def itn_row(itn) -> int:
    """sensevoice_small_model.py:277: an unknown text-norm value is `woitn`."""
    return TEXTNORM_DICT.get(itn, 15) if isinstance(itn, str) else 15


def query_ids(infos, B: int) -> np.ndarray:
    """(B, 4) int32 rows of the embedding table: lid | event | emotion | itn.  Each of
    infos['lid'] / infos['itn'] is one string for the batch (the reference) or a list with one
    entry per utterance."""
    infos = infos or {}
    out = np.zeros((B, N_QUERY), dtype=np.int32)
    out[:, 1], out[:, 2] = EVENT_ROW, EMOTION_ROW
    for col, key, default, row in ((0, 'lid', 'auto', lid_row), (3, 'itn', 'woitn', itn_row)):
        v = infos.get(key, default)
        if isinstance(v, (list, tuple)):
            if len(v) != B:
                raise ValueError(f"infos[{key!r}] has {len(v)} entries for {B} utterances")
            out[:, col] = [row(x) for x in v]
        else:
            out[:, col] = row(v)
    return out


# key -> (required value, the reference's default when the key is missing)
_ENC = dict(input_layer=('paraformer_dummy', 'conv2d'),
            pos_enc_layer_type=('abs_pos_paraformer', 'abs_pos'),
            normalize_before=(True, True), sanm_shfit=(0, 0), static_chunk_size=(0, 0),
            use_dynamic_chunk=(False, False), use_dynamic_left_chunk=(False, False))


def sensevoice_config_from_yaml(configs: dict):
    """train.yaml dict of a `model: sensevoice_small` package -> (wn_config,
    wn_sensevoice_config).  Exactly what the reference's converter writes has kernels; every
    other value is refused by key name.  Dropout rates and `gradient_checkpointing` do not change
    what is computed and are ignored."""
    if configs.get('model') != 'sensevoice_small':
        _refuse('model', configs.get('model', 'asr_model'), 'sensevoice_small')
    if configs.get('encoder') != 'sanm_encoder_with_tp':
        _refuse('encoder', configs.get('encoder', 'conformer'), 'sanm_encoder_with_tp')
    if configs.get('decoder', 'bitransformer') is not None:
        _refuse('decoder', configs.get('decoder', 'bitransformer'), None)
    if configs.get('cmvn') != 'global_cmvn':     # sensevoice_small_model.py:180: asserted there
        _refuse('cmvn', configs.get('cmvn'), 'global_cmvn')
    ec = configs['encoder_conf']
    for k, (want, default) in _ENC.items():
        got = ec.get(k, default)
        if got != want:
            _refuse(f'encoder_conf.{k}', got, want)
    if 'tp_blocks' not in ec or int(ec['tp_blocks']) < 0:
        _refuse('encoder_conf.tp_blocks', ec.get('tp_blocks'), 'a block count')
    d, heads = ec.get('output_size', 256), ec.get('attention_heads', 4)
    if d % heads != 0 or d // heads not in (64, 128):
        _refuse('encoder_conf.output_size / attention_heads', d / heads, '64 or 128')
    K = ec.get('kernel_size', 11)
    if K % 2 != 1 or not 1 <= K <= 63:
        _refuse('encoder_conf.kernel_size', K, 'an odd size up to 63')
    F = ec.get('linear_units', 2048)
    if F % 32 != 0:
        _refuse('encoder_conf.linear_units', F, 'a multiple of 32')
    if configs['input_dim'] != 560:      # sensevoice_small_model.py:178: the table is 560 wide
        _refuse('input_dim', configs['input_dim'], 560)
    lc = configs.get('lfr_conf') or {}
    if lc.get('lfr_m', LFR_M) != LFR_M or lc.get('lfr_n', LFR_N) != LFR_N:
        _refuse('lfr_conf', lc, {'lfr_m': LFR_M, 'lfr_n': LFR_N})
    st = (configs.get('tokenizer_conf') or {}).get('special_tokens') or {}
    if '<s>' not in st or '</s>' not in st:      # sensevoice_small_model.py:169-170
        _refuse('tokenizer_conf.special_tokens', st, "{'<s>': ..., '</s>': ...}")
    mc = configs.get('model_conf') or {}
    if mc.get('ctc_weight', 0.5) == 0.0:          # sensevoice_small_model.py:163
        _refuse('model_conf.ctc_weight', mc.get('ctc_weight'), 'a weight other than 0')
    blank = (configs.get('ctc_conf') or {}).get('ctc_blank_id', 0)
    if blank != 0:
        _refuse('ctc_conf.ctc_blank_id', blank, 0)
    c = _lib.WnConfig()
    c.feat_dim = configs['input_dim'] // LFR_M
    c.d_model, c.n_heads = d, heads
    c.ffn_dim = F
    c.n_layers = ec.get('num_blocks', 6)
    c.cnn_kernel = K
    c.causal = c.use_dynamic_chunk = c.static_chunk_size = 0
    c.vocab = configs['output_dim']
    c.has_cmvn = 1
    c.dec_heads = heads
    c.dec_ffn_dim = F
    c.dec_layers = 0                      # (no attention decoder: ASRModel's modes are off)
    c.dec_r_layers = c.bidirectional = 0
    c.sos, c.eos = st['<s>'], st['</s>']
    c.max_pos = 5000
    c.norm_eps = 1e-5
    c.encoder_type = c.input_layer = c.activation = 0
    p = _lib.WnSenseVoiceConfig()
    p.lfr_m, p.lfr_n = LFR_M, LFR_N
    p.kernel_size = K
    p.tp_blocks = int(ec['tp_blocks'])
    p.max_frames = MAX_FRAMES
    p.n_query, p.n_embed = N_QUERY, N_EMBED
    return c, p


class SenseVoiceSmall(ASRModel):
    """SenseVoice Small with the reference's inference API; `ctc_greedy_search` is its decode
    method."""

    default_decode_method = 'ctc_greedy_search'   # sensevoice_small_model.py:144

    def __init__(self, configs: dict, state_dict: Dict[str, torch.Tensor], device='cuda'):
        # `encoder.embed.pos_enc.pe` is a buffer: the library rebuilds the rows it keeps in fp64.
        # The model takes the CMVN off its encoder (sensevoice_small_model.py:180-182): its own
        # state dict says `global_cmvn.*`; a package whose CMVN comes from the json file arrives
        # with the encoder's names
        sd = {}
        for k, v in state_dict.items():
            if k == 'encoder.embed.pos_enc.pe':
                continue
            if k.startswith('encoder.global_cmvn.'):
                k = k[len('encoder.'):]
            sd[k] = v
        super().__init__(configs, sd, device)
        self.default_decode_method = 'ctc_greedy_search'

    def _config(self, configs: dict) -> _lib.WnConfig:
        cfg, self._scfg = sensevoice_config_from_yaml(configs)
        return cfg

    def _create(self, L, tensors, n: int, h) -> int:
        return L.wn_model_create_sensevoice(ctypes.byref(self._cfg), ctypes.byref(self._scfg),
                                            tensors, n, self.device.index, ctypes.byref(h))

    def clone(self):
        raise NotImplementedError('clone() is outside the accelerated path of a SenseVoice model')

    def set_compute_dtype(self, dtype) -> 'SenseVoiceSmall':
        if self._DTYPES.get(dtype, -1) != 0:
            raise NotImplementedError(
                f'compute dtype {dtype!r} is outside the accelerated path: a SenseVoice model '
                "stays 'fp32'")
        return super().set_compute_dtype(dtype)

    def subsampling_rate(self) -> int:
        return LFR_N

    def right_context(self) -> int:
        return LFR_M - 1 - (LFR_M - 1) // 2

    def _check_simulate_streaming(self, speech):
        raise NotImplementedError('simulate_streaming is outside the accelerated path: the '
                                  'SenseVoice encoder attends over the full utterance')

    def forward_encoder_chunk(self, *args, **kwargs):
        raise NotImplementedError('forward_encoder_chunk is outside the accelerated path: the '
                                  'SenseVoice encoder attends over the full utterance')

    forward_encoder_chunk_batch = forward_encoder_chunk
    forward_encoder_chunk_by_chunk = forward_encoder_chunk

    def align(self, *args, **kwargs):
        raise NotImplementedError('align is outside the accelerated path of a SenseVoice model: '
                                  'the four query frames in front of every utterance would '
                                  'shift the frame times')

    align_wav = align

    def _encode(self, speech, lens, chunk, left, want_out: bool, qid=None):
        """`qid`: (B, 4) int32 query rows of this encode (None: auto / woitn).  Every utterance
        has frames (`_with_frames` takes the others out first)."""
        if chunk > 0 or left > 0:
            raise NotImplementedError(
                'decoding_chunk_size / num_decoding_left_chunks are outside the accelerated '
                'path: the SenseVoice encoder attends over the full utterance')
        B, T, F = speech.shape
        assert F == self._cfg.feat_dim, 'feature dimension mismatch (fbank frames, before LFR)'
        Tp = out_len(T)
        enc_lens = np.zeros((B, ), dtype=np.int32)
        out = None
        if want_out:
            out = torch.empty((B, Tp, self._cfg.d_model), dtype=torch.float32, device=self.device)
        qid = np.ascontiguousarray(query_ids(None, B) if qid is None else qid, dtype=np.int32)
        assert qid.shape == (B, N_QUERY)
        _lib.check(self._L.wn_sensevoice_set_queries(self._h, _lib.i32p(qid), B),
                   'wn_sensevoice_set_queries')
        _lib.check(
            self._L.wn_encode(self._h, speech.data_ptr(), _lib.i32p(lens), B, T, -1, -1,
                              out.data_ptr() if out is not None else None, _lib.i32p(enc_lens),
                              _stream_ptr(self.device)), 'wn_encode')
        return out, enc_lens, Tp

    def _with_frames(self, speech, lens, qid):
        """The utterances that have frames, as a batch of their own: (indices, speech, lens,
        qid).  One without frames has no encoder rows and an empty result (the reference raises
        inside LFR), so it never reaches the library."""
        keep = np.nonzero(lens > 0)[0]
        if keep.size == lens.shape[0]:
            return keep, speech, lens, qid
        idx = torch.as_tensor(keep, device=speech.device, dtype=torch.long)
        return (keep, speech.index_select(0, idx).contiguous(), np.ascontiguousarray(lens[keep]),
                np.ascontiguousarray(qid[keep]))

    def _forward_encoder(self, speech, speech_lengths, decoding_chunk_size: int = -1,
                         num_decoding_left_chunks: int = -1, simulate_streaming: bool = False,
                         infos=None):
        """-> (encoder_out (B, T', d), encoder_mask (B, 1, T')) of fbank frames under the query
        rows of `infos` (as in decode; None: auto / woitn); T' counts the four query frames."""
        if simulate_streaming:
            self._check_simulate_streaming(speech)
        speech, lens = self._prep(speech, speech_lengths)
        B, Tp = speech.shape[0], out_len(speech.shape[1])
        keep, sp, ln, qid = self._with_frames(speech, lens, query_ids(infos, B))
        enc_lens = np.zeros((B, ), dtype=np.int32)
        out = torch.zeros((B, Tp, self._cfg.d_model), dtype=torch.float32, device=self.device)
        if keep.size > 0:
            o, el, _ = self._encode(sp, ln, decoding_chunk_size, num_decoding_left_chunks, True,
                                    qid)
            enc_lens[keep] = el
            out = o if keep.size == B else out.index_copy_(
                0, torch.as_tensor(keep, device=self.device, dtype=torch.long), o)
        mask = (torch.arange(Tp, device=self.device).unsqueeze(0) <
                torch.as_tensor(enc_lens, device=self.device).unsqueeze(1))
        return out, mask.unsqueeze(1)

    def decode(self, methods: List[str], speech, speech_lengths, beam_size: int = 1,
               decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
               ctc_weight: float = 0.0, simulate_streaming: bool = False,
               reverse_weight: float = 0.0, context_graph=None, blank_id: int = 0,
               blank_penalty: float = 0.0, length_penalty: float = 0.0,
               infos=None) -> Dict[str, List[DecodeResult]]:
        """sensevoice_small_model.py:249-290, then asr_model.py:267-343 for the two CTC methods.
        Token lists hold whatever the four query frames emit, and `times` count those frames,
        as in the reference."""
        for m in methods:
            if m not in METHODS:
                raise NotImplementedError(
                    f'decode method {m!r} is outside the accelerated path of a SenseVoice model: '
                    f'it has no attention decoder (has: {", ".join(METHODS)})')
        if simulate_streaming:
            self._check_simulate_streaming(speech)
        assert decoding_chunk_size != 0
        speech, lens = self._prep(speech, speech_lengths)    # (a copy: the caller's stay)
        B = speech.shape[0]
        keep, sp, ln, qid = self._with_frames(speech, lens, query_ids(infos, B))
        results = {m: [DecodeResult([], times=[]) for _ in range(B)] for m in methods}
        if keep.size == 0:
            return results
        self._use_context_graph(context_graph)
        _, enc_lens, Tp = self._encode(sp, ln, decoding_chunk_size, num_decoding_left_chunks,
                                       False, qid)
        need_beam = 'ctc_prefix_beam_search' in methods
        _lib.check(
            self._L.wn_ctc_logprobs(self._h, beam_size if need_beam else 1, blank_id,
                                    blank_penalty, None, Tp, _stream_ptr(self.device)),
            'wn_ctc_logprobs')
        st = dict(methods=list(methods), B=int(keep.size), enc_lens=enc_lens,
                  need_beam=need_beam, beam_size=beam_size, blank_id=blank_id, speech=sp, Tp=Tp)
        got = self._decode_end(st, 0.0, 0.0, length_penalty, None)
        for m in methods:
            for j, b in enumerate(keep):
                results[m][int(b)] = got[m][j]
        return results
