"""Token id <-> text for the result writer (the decode path only needs ids).

Mirrors what `init_tokenizer(configs)` (wenet/utils/init_tokenizer.py:26-60)
hands to `recognize.py` / the CLI for the two tokenizers the Conformer recipes
use:
  * `char`: CharTokenizer.detokenize = connect_symbol.join(symbols)
    (wenet/text/char_tokenizer.py:56-57, base_tokenizer.py:14-17);
  * `bpe`:  BpeTokenizer.detokenize = the same join with the sentencepiece
    word-boundary mark turned into spaces and stripped (bpe_tokenizer.py:48-51).
Text -> ids (training side) is out of scope, except for the biasing phrase list
(wenet_amd/context_graph.py).
"""
import os
from typing import Dict, List, Tuple


def read_symbol_table(path: str) -> Dict[str, int]:
    """wenet/utils/file_utils.py:61-68: `symbol id` per line."""
    table = {}
    with open(path, 'r', encoding='utf8') as f:
        for line in f:
            arr = line.strip().split()
            assert len(arr) == 2, f'bad symbol table line: {line!r}'
            table[arr[0]] = int(arr[1])
    return table


_PF_DROPPED = ('<sos>', '<eos>', '<blank>')
_PF_MARKS = (' ', '</s>', '<s>', '<unk>', '<OOV>')


def _pf_strip(token: str) -> str:
    for mark in _PF_MARKS:
        token = token.replace(mark, '')
    return token


def _pf_is_han(piece: str) -> bool:
    """One piece counts as Chinese when, as a string, it lies inside the CJK block, inside the
    digits, or is '@' (paraformer/search.py:11-14: a range comparison of the whole string)."""
    return '一' <= piece <= '鿿' or '0' <= piece <= '9' or piece == '@'


def _pf_all_han(pieces) -> bool:
    """paraformer/search.py:17-33 over the pieces of `pieces` (the tokens of a list, or the
    characters of one token)."""
    cleaned = [_pf_strip(p) for p in pieces]
    return len(cleaned) > 0 and all(_pf_is_han(p) for p in cleaned)


def _pf_all_alpha(pieces) -> bool:
    """paraformer/search.py:36-55: letters (not Chinese ones) and apostrophes only."""
    cleaned = [_pf_strip(p) for p in pieces]
    if not cleaned:
        return False
    for p in cleaned:
        if p.isalpha():
            if _pf_is_han(p):
                return False
        elif p != "'":
            return False
    return True


def paraformer_tokens2text(tokens: List[str]) -> str:
    """The rule of paraformer_beautify_result (paraformer/search.py:58-111) restated: special
    tokens dropped; an all-Chinese list is joined as it is; an all-alphabetic list joins '@@'
    pieces to the piece behind them and puts a space behind every finished word; a mixed list
    does both, and a Chinese token takes back the space behind the word in front of it."""
    kept = [t for t in tokens if t not in _PF_DROPPED]
    out: List[str] = []
    word = ''
    if _pf_all_han(kept):
        out = [t.replace(' ', '') for t in kept]
    elif _pf_all_alpha(kept):
        for t in kept:
            if '@@' in t:
                word += t.replace('@@', '')
            else:
                out += [word + t, ' ']
                word = ''
    else:
        space_pending = False
        for t in kept:
            if _pf_all_han(t):
                if space_pending:
                    out.pop()
                out.append(t)
                space_pending = False
            elif '@@' in t:
                word += t.replace('@@', '')
                space_pending = False
            elif _pf_all_alpha(t):
                out += [word + t, ' ']
                word = ''
                space_pending = True
            else:
                out.append(t)
                space_pending = False
    return ''.join(out).strip()


class Tokenizer:

    def __init__(self, symbol_table, kind: str = 'char', connect_symbol: str = '',
                 bpe_path: str = None):
        if not isinstance(symbol_table, dict):
            symbol_table = read_symbol_table(symbol_table)
        assert kind in ('char', 'bpe', 'paraformer')
        self.kind = kind
        self.connect_symbol = connect_symbol if kind == 'char' else ''
        self.bpe_path = bpe_path
        self._symbol_table = symbol_table
        self.char_dict = {v: k for k, v in symbol_table.items()}

    @property
    def symbol_table(self) -> Dict[str, int]:
        return self._symbol_table

    def vocab_size(self) -> int:
        return len(self.char_dict)

    def ids2tokens(self, ids: List[int]) -> List[str]:
        return [self.char_dict[int(w)] for w in ids]  # KeyError like the reference

    def tokens2text(self, tokens: List[str]) -> str:
        if self.kind == 'paraformer':   # paraformer_tokenizer.py:52-53 (detokenising only)
            return paraformer_tokens2text(tokens)
        text = self.connect_symbol.join(tokens)
        if self.kind == 'bpe':
            text = text.replace('▁', ' ').strip()
        return text

    def detokenize(self, ids: List[int]) -> Tuple[str, List[str]]:
        tokens = self.ids2tokens(ids)
        return self.tokens2text(tokens), tokens


def init_tokenizer(configs: dict, model_dir: str = None) -> Tokenizer:
    """init_tokenizer for `tokenizer: char | bpe`; with `model_dir`, paths of
    tokenizer_conf are first looked up next to the model like
    wenet/cli/model.py:41-45."""
    kind = configs.get('tokenizer', 'char')
    if kind not in ('char', 'bpe', 'paraformer'):
        raise NotImplementedError(f'tokenizer {kind!r} (char, bpe and paraformer are supported)')
    conf = dict(configs['tokenizer_conf'])
    if model_dir is not None:
        for key, value in conf.items():
            if isinstance(value, str):
                local = os.path.join(model_dir, os.path.basename(value))
                if os.path.exists(local):
                    conf[key] = local
    return Tokenizer(conf['symbol_table_path'], kind,
                     connect_symbol=conf.get('connect_symbol', ''),
                     bpe_path=conf.get('bpe_path'))


def get_blank_id(configs: dict, symbol_table: Dict[str, int]) -> int:
    """wenet/utils/ctc_utils.py:122-136."""
    ctc_conf = configs.setdefault('ctc_conf', {})
    if '<blank>' in symbol_table:
        if 'ctc_blank_id' in ctc_conf:
            assert ctc_conf['ctc_blank_id'] == symbol_table['<blank>']
        else:
            ctc_conf['ctc_blank_id'] = symbol_table['<blank>']
    else:
        assert 'ctc_blank_id' in ctc_conf, 'PLZ set ctc_blank_id in yaml'
    return ctc_conf['ctc_blank_id']
