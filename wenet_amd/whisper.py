"""The Whisper prompt of the `attention` decode mode.

The reference starts every hypothesis of a Whisper model from the tokens
`add_whisper_tokens(no_timestamp=True, use_prev=False)` builds
(wenet/utils/common.py:159-238, called from attention_beam_search,
wenet/models/transformer/search.py:267-289):

    transcribe / translate:  [sot, sot + 1 + language index, task, no_timestamps]
    vad:                     [sot, sot + 1 + language index, no_speech, no_speech]

The language index is the position of the code in the `whisper` package's LANGUAGES table;
`WHISPER_LANGS` is that table's key order as Whisper publishes it.  Only `en` = 0 and `zh` = 1
are pinned to the reference harness (tests/golden/whisperdec_*.npz); the other 98 positions are
parity unpinned.
"""
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

WHISPER_LANGS = (
    'en', 'zh', 'de', 'es', 'ru', 'ko', 'fr', 'ja', 'pt', 'tr', 'pl', 'ca', 'nl', 'ar', 'sv',
    'it', 'id', 'hi', 'fi', 'vi', 'he', 'uk', 'el', 'ms', 'cs', 'ro', 'da', 'hu', 'ta', 'no',
    'th', 'ur', 'hr', 'bg', 'lt', 'la', 'mi', 'ml', 'cy', 'sk', 'te', 'fa', 'lv', 'bn', 'sr',
    'az', 'sl', 'kn', 'et', 'mk', 'br', 'eu', 'is', 'hy', 'ne', 'mn', 'bs', 'kk', 'sq', 'sw',
    'gl', 'mr', 'pa', 'si', 'km', 'sn', 'yo', 'so', 'af', 'oc', 'ka', 'be', 'tg', 'sd', 'gu',
    'am', 'yi', 'lo', 'uz', 'fo', 'ht', 'ps', 'tk', 'nn', 'mt', 'sa', 'lb', 'my', 'bo', 'tl',
    'mg', 'as', 'tt', 'haw', 'ln', 'ha', 'ba', 'jw', 'su', 'yue')

_TASKS = {'transcribe': 'transcribe', 'translate': 'translate', 'vad': 'no_speech'}


def is_whisper(special_tokens: Optional[dict]) -> bool:
    """search.py:267-268: the model takes the Whisper branch of attention_beam_search."""
    return special_tokens is not None and 'transcribe' in special_tokens


def language_index(lang: Union[str, int]) -> int:
    """Position of a language code in WHISPER_LANGS; an int is taken as the index itself."""
    if isinstance(lang, (int, np.integer)) and not isinstance(lang, bool):
        if not 0 <= int(lang) < len(WHISPER_LANGS):
            raise ValueError(f'language index {lang} outside [0, {len(WHISPER_LANGS)})')
        return int(lang)
    try:
        return WHISPER_LANGS.index(lang)
    except ValueError:
        raise ValueError(f'unknown Whisper language code {lang!r}') from None


def prompt_row(special_tokens: dict, task: str, lang: Union[str, int]) -> List[int]:
    """The prompt of one utterance (common.py:199-221)."""
    if task not in _TASKS:
        raise NotImplementedError('unsupported task {}'.format(task))
    sot = special_tokens['sot']
    task_id = special_tokens[_TASKS[task]]
    last = special_tokens['no_speech'] if task == 'vad' else special_tokens['no_timestamps']
    return [sot, sot + 1 + language_index(lang), task_id, last]


def build_prompts(special_tokens: dict, batch_size: int,
                  infos: Optional[Dict[str, Sequence]] = None) -> np.ndarray:
    """(B, 4) int32 prompts; infos = None: `transcribe` / `en` for every utterance
    (search.py:269-272)."""
    if infos is None:
        tasks, langs = ['transcribe'] * batch_size, ['en'] * batch_size
    else:
        tasks, langs = list(infos['tasks']), list(infos['langs'])
    if len(tasks) != batch_size or len(langs) != batch_size:
        raise ValueError(f"infos: {len(tasks)} tasks / {len(langs)} langs for a batch of "
                         f'{batch_size} utterances')
    return np.asarray([prompt_row(special_tokens, t, l) for t, l in zip(tasks, langs)],
                      dtype=np.int32).reshape(batch_size, 4)
