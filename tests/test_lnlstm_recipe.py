"""CPU tests of the `layer_norm` cfg key and of the variables layer.blstm(layer_norm=True) creates.  No GPU: the store
lives on the CPU, the layer creates its variables, sizes the call on the host and then refuses the CPU tensors at the
first kernel call (the HIP path has no CPU fallback) — what exists by then is what is checked."""
import os

import numpy as np
import pytest
import torch

from nabu_amd import recipes, variables as vs, _hip
from nabu_amd.neuralnetworks.components import layer
from nabu_amd.neuralnetworks.models.ed_encoders.listener import layer_norm_key
from tests import lnlstm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def created_by_layer(layer_norm, D=8, H=16):
    from nabu_amd import build
    build.build(verbose=False)
    store = vs.VariableStore(seed=0, device=torch.device('cpu'))
    with vs.as_default(store):
        with pytest.raises(_hip.NabuHipError, match='not on the GPU'):
            layer.blstm(torch.zeros(2, 5, D), np.array([5, 3], np.int32), H, layer_norm=layer_norm, scope='L')
    return store


def test_cfg_key_is_parsed_and_defaults_to_false():
    assert layer_norm_key({}) is False
    assert layer_norm_key({'layer_norm': 'True'}) is True and layer_norm_key({'layer_norm': 'False'}) is False
    with pytest.raises(ValueError):
        layer_norm_key({'layer_norm': 'yes'})
    mc, _, _ = recipes.load_recipe('cfg2_listener_ctc', **{'encoder.layer_norm': 'True'})
    assert layer_norm_key(dict(mc.items('encoder'))) is True


def test_no_shipped_recipe_or_defaults_file_turns_it_on():
    for recipe in sorted(os.listdir(recipes.RECIPES)):
        if not os.path.isdir(os.path.join(recipes.RECIPES, recipe)):
            continue
        mc, _, _ = recipes.load_recipe(recipe)
        if mc.get('encoder', 'encoder') not in ('listener', 'dblstm'):      # (the DNN encoder has a key of its own by this name)
            continue
        assert layer_norm_key(dict(mc.items('encoder'))) is False, recipe
    for name in ('listener.cfg', 'dblstm.cfg'):        # read with conf.get: the defaults files keep their key set
        f = os.path.join(ROOT, 'nabu_amd', 'neuralnetworks', 'models', 'ed_encoders', 'defaults', name)
        assert 'layer_norm' not in open(f).read(), f


def test_default_false_creates_kernel_and_bias_only():
    store = created_by_layer(False)
    assert store.order == ['L/' + (R.CELL % d) + '/' + w for d in ('fw', 'bw') for w in ('kernel', 'bias')]


def test_true_creates_the_norm_variables_and_no_bias():
    store = created_by_layer(True)
    assert [(n, store.vars[n].shape) for n in store.order] == [('L/' + n, s) for n, s in R.variable_shapes(8, 16)]
    assert not any(n.endswith('bias') for n in store.order)
    for n in store.order:
        if n.endswith('gamma'):
            assert (store.vars[n].data == 1).all()
        if n.endswith('beta'):
            assert (store.vars[n].data == 0).all()


def test_encoders_pass_the_key_to_every_layer(monkeypatch):
    from nabu_amd.neuralnetworks.models.ed_encoders import listener, dblstm
    seen = []

    def fake_blstm(inputs, sequence_length, num_units, layer_norm=False, scope=None, out_stack=0):
        seen.append(layer_norm)
        return inputs

    def fake_pblstm(inputs, sequence_length, num_units, num_steps=2, layer_norm=False, scope=None):
        seen.append(layer_norm)
        return inputs, sequence_length
    monkeypatch.setattr(layer, 'blstm', fake_blstm)
    monkeypatch.setattr(layer, 'pblstm', fake_pblstm)
    for cls, n in ((listener.Listener, 4), (dblstm.DBLSTM, 3)):
        for value in ('True', 'False'):
            del seen[:]
            enc = cls.__new__(cls)
            enc.conf = {'num_layers': '3', 'num_units': '8', 'pyramid_steps': '2', 'input_noise': '0', 'dropout': '1',
                        'layer_norm': value}
            enc.encode({'features': torch.zeros(2, 4, 3)}, {'features': np.array([4, 2])}, False)
            assert seen == [value == 'True'] * n, (cls.__name__, value, seen)
