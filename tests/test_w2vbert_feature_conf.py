"""bin/recognize.py accepts the W2v-BERT feature recipe (`feats_type: w2vbert_fbank`) under the
checks of the fbank branch, and keeps every other refusal."""
import pytest

from wenet_amd import synthetic as S
from wenet_amd.bin import recognize as R


def _cfg(**conf):
    c = S.make_configs('tiny_shaw_w2vbert')
    c['dataset_conf']['w2vbert_fbank_conf'].update(conf)
    return c


def test_recipe_is_accepted_and_dispatched():
    cfg = _cfg()
    R.check_feature_conf(cfg)

    class M:
        compute_fbank = staticmethod(lambda waves: ('fbank', waves))
        compute_w2vbert_fbank = staticmethod(lambda waves: ('w2vbert_fbank', waves))
    fn, frames_of = R.feature_function(M, cfg)
    assert fn(['w']) == ('w2vbert_fbank', ['w'])
    assert [frames_of(n) for n in (399, 400, 560, 160000)] == [0, 1, 2, 998]
    assert R.feature_function(M, S.make_configs('tiny_shaw'))[0](['w']) == ('fbank', ['w'])


@pytest.mark.parametrize('conf', [dict(frame_length=20), dict(frame_shift=20),
                                  dict(num_mel_bins=23)], ids=str)
def test_wrong_frames_are_refused_as_for_fbank(conf):
    with pytest.raises(NotImplementedError, match='fbank must be 25 ms / 10 ms frames with '
                                                  'input_dim mel bins'):
        R.check_feature_conf(_cfg(**conf))


def test_mfcc_stays_refused():
    with pytest.raises(NotImplementedError, match='fbank or log_mel_spectrogram features only'):
        R.check_feature_conf({'dataset_conf': {'feats_type': 'mfcc'}})
