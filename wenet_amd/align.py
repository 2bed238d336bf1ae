"""CTC forced alignment: `force_align` of wenet/utils/ctc_utils.py:106 and the time-stamp
helpers of wenet/bin/alignment.py on the MI355X path.

The alignment itself (emission gather + Viterbi trellis + backtrace) runs in
`wn_ctc_force_align` (csrc/ctc_align.hip); what is here is the host side: argument packing,
the pure list walks `get_frames_timestamp` / `get_labformat` restated with their script globals
as arguments, and a plain-text TextGrid writer.

The rule of the trellis: fp32, ties to the earlier candidate (stay, then
step, then skip), the last label ends the path unless the trailing blank is strictly better.
torchaudio's forced_align (what the reference calls) is not pinned on ties.
"""
import ctypes
import math
import re
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

__all__ = ['AlignResult', 'force_align', 'force_align_batch', 'align_current_batch',
           'get_frames_timestamp', 'get_labformat', 'get_intervals', 'format_textgrid',
           'write_textgrid', 'tokenize_text']


@dataclass
class AlignResult:
    """One utterance of ASRModel.align.  `alignment`: the label id of every encoder frame (T'
    entries, blank between tokens); `score`: the path's log-probability; `ok`: False when the
    label list does not fit into the frames (everything else is empty then); `frames`: the
    token groups of get_frames_timestamp; `intervals`: (begin_s, end_s, token_id) per group,
    the numbers get_labformat prints."""
    tokens: List[int]
    alignment: List[int] = field(default_factory=list)
    score: float = float('-inf')
    ok: bool = False
    frames: List[List[int]] = field(default_factory=list)
    intervals: List[Tuple[float, float, int]] = field(default_factory=list)


# ---- host restatements of bin/alignment.py ---------------------------------------------------

def get_frames_timestamp(alignment: Sequence[int], prob, blank_thres: float = 0.999,
                         thres: float = 0.0000000001, blank_id: int = 0) -> List[List[int]]:
    """alignment.py:55-85: split the per-frame alignment into one group of frames per token
    (leading blanks, then the token's frames; trailing blanks join the last group) and pull a
    token's front border forward over the frames in front of it whose blank log-prob is under
    log(blank_thres) or whose log-prob of the token is over log(thres).  `prob[t][id]` is read
    for id = blank and id = the group's token only.  The reference hard-codes blank 0 and
    changes `alignment` in place; here the blank is an argument and the caller's list stays."""
    alignment = [int(a) for a in alignment]
    n = len(alignment)
    # the two log-probs of a frame the walk can read: blank, and the token of the group the
    # frame belongs to (the next label at or behind it)
    if isinstance(prob, _TwoColumns):
        pb, pt = prob.fl[:n, 0].tolist(), prob.fl[:n, 1].tolist()
    else:
        pb, pt, grp = [0.0] * n, [0.0] * n, blank_id
        for t in range(n - 1, -1, -1):
            if alignment[t] != blank_id:
                grp = alignment[t]
            row = prob[t]
            pb[t], pt[t] = float(row[blank_id]), float(row[grp])
    log_blank, log_thres = math.log(blank_thres), math.log(thres)
    timestamp: List[List[int]] = []
    start = end = 0
    while end < n:
        while end < n and alignment[end] == blank_id:
            end += 1
        if end == n:
            if not timestamp:       # nothing but blanks (the reference fails here)
                return []
            timestamp[-1] += alignment[start:]
            break
        end += 1
        while end < n and alignment[end - 1] == alignment[end]:
            end += 1
        local_start = end - 1
        token = alignment[end - 1]
        while local_start >= start and (pb[local_start] < log_blank
                                        or pt[local_start] > log_thres):
            alignment[local_start] = token
            local_start -= 1
        timestamp.append(alignment[start:end])
        start = end
    return timestamp


def get_intervals(timestamp: Sequence[Sequence[int]], subsample: int, blank_id: int = 0
                  ) -> List[Tuple[float, float, int]]:
    """The numbers of alignment.py:88-123 get_labformat: (begin, end, token id) per group in
    seconds -- 10 ms frame shift times the subsampling rate per encoder frame; the same float
    operations in the same order, so that formatting them gives the reference's lines."""
    out = []
    begin_time = 0
    for idx, t in enumerate(timestamp):
        i = 0
        while t[i] == blank_id:
            i += 1
        begin = i
        dur = 0
        while i < len(t) and t[i] != blank_id:
            i += 1
            dur += 1
        begin = begin_time + begin * 0.01 * subsample
        duration = dur * 0.01 * subsample
        if idx < len(timestamp) - 1:
            token = t[-1]
        else:   # the last group carries the trailing blanks
            token = next(x for x in t if x != blank_id)
        out.append((begin, begin + duration, int(token)))
        begin_time += len(t) * 0.01 * subsample
    return out


def get_labformat(timestamp: Sequence[Sequence[int]], subsample: int,
                  char_dict: Optional[Dict[int, str]] = None, blank_id: int = 0) -> List[str]:
    """alignment.py:88-123: one `begin end token` line per group ('%.2f %.2f %s\\n').  The
    reference reads `configs` and `char_dict` as script globals and prints each line as well;
    here they are arguments and nothing is printed.  Without `char_dict` the id is written."""
    return ['{:.2f} {:.2f} {}\n'.format(b, e, char_dict[tok] if char_dict is not None else tok)
            for b, e, tok in get_intervals(timestamp, subsample, blank_id)]


def format_textgrid(maxtime: float, lines: Sequence[str], margin: float = 0.0001) -> str:
    """A Praat TextGrid (long text format) with one interval tier "line" holding the `.lab`
    lines, the gaps between them as empty intervals -- what alignment.py:37-52 builds with the
    `textgrid` package (minTime = begin + margin).  Written here as plain text; parity with
    that package's writer is not pinned."""
    marks = []
    for ln in lines:
        s, e, w = ln.split()
        marks.append((float(s) + margin, float(e), w))
    ivs, cur = [], 0.0
    for s, e, w in marks:
        if s > cur:
            ivs.append((cur, s, ''))
        ivs.append((s, e, w))
        cur = e
    if cur < maxtime:
        ivs.append((cur, maxtime, ''))
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', '', 'xmin = 0',
           f'xmax = {maxtime}', 'tiers? <exists>', 'size = 1', 'item []:', '    item [1]:',
           '        class = "IntervalTier"', '        name = "line"', '        xmin = 0',
           f'        xmax = {maxtime}', f'        intervals: size = {len(ivs)}']
    for i, (s, e, w) in enumerate(ivs, 1):
        w = w.replace('"', '""')
        out += [f'        intervals [{i}]:', f'            xmin = {s}', f'            xmax = {e}',
                f'            text = "{w}"']
    return '\n'.join(out) + '\n'


def write_textgrid(path: str, maxtime: float, lines: Sequence[str]) -> None:
    with open(path, 'w', encoding='utf8') as f:
        f.write(format_textgrid(maxtime, lines))


_CJK = re.compile(r'([一-鿿])')


def tokenize_text(text: str, symbol_table: Dict[str, int], bpe_model: Optional[str] = None,
                  kind: Optional[str] = None) -> List[int]:
    """Transcript -> label ids: char units map ' ' to U+2581; with a BPE model the text is
    upper-cased, CJK characters stay single tokens and the rest goes through sentencepiece
    (text/tokenize_utils.py).  Symbols missing from the table become <unk> when the table has
    one and are dropped otherwise."""
    if bpe_model is not None and kind != 'char':
        import sentencepiece as spm
        sp = spm.SentencePieceProcessor()
        sp.load(bpe_model)
        units = []
        for piece in _CJK.split(text.strip().upper()):
            if not piece.strip():
                continue
            if _CJK.fullmatch(piece):
                units.append(piece)
            else:
                units.extend(sp.encode_as_pieces(piece))
    else:
        units = ['▁' if ch == ' ' else ch for ch in text.strip()]
    unk = symbol_table.get('<unk>')
    ids = []
    for u in units:
        if u in symbol_table:
            ids.append(symbol_table[u])
        elif unk is not None:
            ids.append(unk)
    return ids


# ---- the device call ---------------------------------------------------------------------------

class _TwoColumns:
    """The (T', 2) frame log-probs of wn_ctc_force_align as get_frames_timestamp's `prob`:
    column 0 the blank's, column 1 that of the token group the frame belongs to -- the only two
    values the walk reads per frame."""

    def __init__(self, fl, blank):
        self.fl, self.blank = np.asarray(fl), blank


def pack_labels(labels: Sequence[Sequence[int]]):
    lens = np.asarray([len(y) for y in labels], np.int32)
    max_label = max(1, int(lens.max()) if len(lens) else 1)
    lab = np.zeros((len(labels), max_label), np.int32)
    for b, y in enumerate(labels):
        lab[b, :len(y)] = np.asarray(list(y), np.int64)
    return lab, lens, max_label


def _call(L, handle, stream, labels, blank_id, blank_penalty, B, Tp, V, logp_ptr, lens,
          want_frames: bool, want_emit: bool):
    from wenet_amd import _lib
    lab, lab_lens, max_label = pack_labels(labels)
    assert lab.shape[0] == B, 'one label list per utterance'
    path = np.full((B, Tp), -1, np.int32)
    score = np.full((B, ), -np.inf, np.float32)
    status = np.zeros((B, ), np.int32)
    fl = np.zeros((B, Tp, 2), np.float32) if want_frames else None
    emit = np.zeros((B, Tp, max_label + 1), np.float32) if want_emit else None
    _lib.check(
        L.wn_ctc_force_align(handle, int(blank_id), float(blank_penalty), _lib.i32p(lab),
                             _lib.i32p(lab_lens), max_label, logp_ptr,
                             _lib.i32p(lens) if lens is not None else None, B, Tp, V,
                             _lib.i32p(path), _lib.f32p(score), _lib.i32p(status),
                             _lib.f32p(fl) if fl is not None else None,
                             _lib.f32p(emit) if emit is not None else None, stream),
        'wn_ctc_force_align')
    return dict(path=path, score=score, status=status, frame_logp=fl, emit=emit,
                label_lens=lab_lens)


def align_current_batch(model, labels, enc_lens, Tp: int, blank_id: int = 0,
                        blank_penalty: float = 0.0, want_emit: bool = False):
    """wn_ctc_force_align on `model`'s current batch (after its encoder ran): the raw arrays."""
    from wenet_amd.search import _stream_ptr
    raw = _call(model._L, model._h, _stream_ptr(model.device), labels, blank_id, blank_penalty,
                len(labels), Tp, 0, None, None, True, want_emit)
    raw['lens'] = np.asarray(enc_lens, np.int32)
    return raw


def force_align_batch(ctc_probs, ctc_lens, labels, blank_id: int = 0, return_raw: bool = False):
    """Forced alignment of many: ctc_probs (B, T, V) normalised log-probs on the GPU, ctc_lens
    (B,), labels a list of B id lists -> list of 1-D int64 alignments (None where the labels do
    not fit into the frames)."""
    import torch
    from wenet_amd import _lib
    from wenet_amd.search import _Workspace, _require_cuda, _stream_ptr
    _require_cuda(ctc_probs, 'force_align')
    assert ctc_probs.dim() == 3
    probs = ctc_probs.detach().to(torch.float32).contiguous()
    B, T, V = probs.shape
    lens = np.ascontiguousarray(torch.as_tensor(ctc_lens).detach().cpu().numpy().astype(np.int32))
    labels = [[int(t) for t in (y.tolist() if hasattr(y, 'tolist') else y)] for y in labels]
    raw = _call(_lib.lib(), _Workspace.handle(probs.device), _stream_ptr(probs.device), labels,
                blank_id, 0.0, B, T, V, ctypes.c_void_p(probs.data_ptr()), lens, False,
                return_raw)
    raw['lens'] = lens
    if return_raw:
        return raw
    return [torch.from_numpy(raw['path'][b, :lens[b]].astype(np.int64))
            if raw['status'][b] == 0 else None for b in range(B)]


def force_align(ctc_probs, y, blank_id: int = 0):
    """ctc_utils.py:106: ctc_probs (T, V) log-probs on the GPU, y 1-D label ids -> the 1-D int64
    alignment (label id per frame).  ValueError when the labels do not fit into T frames."""
    import torch
    assert ctc_probs.dim() == 2
    out = force_align_batch(ctc_probs[None], torch.tensor([ctc_probs.size(0)]), [y], blank_id)
    if out[0] is None:
        raise ValueError(f'force_align: {len(y)} labels (plus a frame between adjacent repeats) '
                         f'do not fit into {ctc_probs.size(0)} frames')
    return out[0]


def results_from_raw(raw, labels, subsample: int, blank_id: int, blank_thres: float,
                     thres: float) -> List[AlignResult]:
    out = []
    for b, y in enumerate(labels):
        r = AlignResult(tokens=[int(t) for t in y])
        if raw['status'][b] == 0:
            n = int(raw['lens'][b])
            r.ok = True
            r.alignment = raw['path'][b, :n].tolist()
            r.score = float(raw['score'][b])
            r.frames = get_frames_timestamp(r.alignment,
                                            _TwoColumns(raw['frame_logp'][b, :n], blank_id),
                                            blank_thres, thres, blank_id)
            r.intervals = get_intervals(r.frames, subsample, blank_id)
        out.append(r)
    return out
