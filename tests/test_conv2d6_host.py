"""Host side of the Conv2dSubsampling6 front end: recipe acceptance, the length formula, the tile
list of conv2d6_patch and the rate / context the streaming code reads.  No GPU."""
import os

import numpy as np
import pytest
import torch
import yaml

from wenet_amd import _lib
from wenet_amd.model import ASRModel, config_from_yaml

RECIPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv2d6', 'recipes')


@pytest.mark.parametrize('name', ['train_conformer.yaml', 'train_u2++_conformer.yaml'])
def test_gigaspeech_recipes_accepted(name):
    with open(os.path.join(RECIPES, name)) as f:
        configs = yaml.safe_load(f)
    configs.update(input_dim=80, output_dim=5002)
    c = config_from_yaml(configs)
    assert (c.input_layer, c.encoder_type, c.d_model, c.n_heads) == (2, 0, 512, 8)
    configs['encoder_conf']['input_layer'] = 'conv2d8'
    with pytest.raises(NotImplementedError, match='input_layer'):
        config_from_yaml(configs)
    configs['encoder_conf'].update(input_layer='conv2d6', output_size=384, attention_heads=6)
    with pytest.raises(NotImplementedError, match='conv2d6'):
        config_from_yaml(configs)


def test_length_formula_is_the_mask_slicing():
    L_ = _lib.lib()
    for n in range(81):
        kept = int(torch.ones(1, 1, n, dtype=torch.bool)[:, :, 2::2][:, :, 4::3].sum())
        assert L_.wn_conv2d6_frames(n) == kept, n
        if n >= 11:
            assert kept == ((n - 1) // 2 - 2) // 3 and 6 * (kept - 1) + 10 < n


@pytest.mark.parametrize('ft', [0, 5, 8, 10])
def test_tiles_cover_every_frame_once(ft):
    L_ = _lib.lib()
    l2 = np.asarray([1, 0, 7, 8, 9, 17, 0, 40, 5, 10, 11], np.int32)
    out = np.full(4 * 64, -1, np.int32)
    n = L_.wn_conv2d6_tiles(_lib.i32p(l2), len(l2), ft, _lib.i32p(out), 64)
    assert 0 < n <= 64
    tiles = out[:4 * n].reshape(n, 4)
    width = int(tiles[:, 2].max())
    assert width == (ft or width) and width in (5, 8, 10)
    off = np.concatenate([[0], np.cumsum(l2)])
    seen = np.zeros(int(l2.sum()), np.int32)
    for u, t0, cnt, g0 in tiles:
        assert 0 < cnt <= width and t0 % width == 0 and t0 + cnt <= l2[u], 'crosses an utterance'
        assert g0 == off[u] + t0
        seen[g0:g0 + cnt] += 1
    assert (seen == 1).all()
    assert L_.wn_conv2d6_tiles(_lib.i32p(l2), len(l2), 7, _lib.i32p(out), 64) == -1


def test_rate_and_context():
    m = ASRModel.__new__(ASRModel)
    m._cfg = _lib.WnConfig()
    m._cfg.input_layer = 2
    assert (m.subsampling_rate(), m.right_context()) == (6, 10)
    assert [m._sub_frames(t) for t in (11, 16, 17, 67)] == [1, 1, 2, 10]
