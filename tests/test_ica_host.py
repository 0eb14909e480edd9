"""ICA without a GPU: the fixture's inputs regenerate, the reference stayed
on the float64 trajectory up to every stored horizon, the inverse's C entry
point rejects bad arguments before any HIP call, and train_dictionary checks
its parameters as the reference does."""
import ctypes

import numpy as np
import pytest
import torch

import ica_data
from helpers import load


@pytest.fixture(scope='module')
def golden():
  return load('ica_training')


@pytest.mark.parametrize('name', sorted(ica_data.CASES))
def test_regenerated_training_inputs_match_the_fixture(golden, name):
  n, nb, seed = ica_data.CASES[name]
  data, mixing = ica_data.batches(n, nb, seed)
  d0 = ica_data.init_dictionary(n, seed)
  assert data.shape == (nb, ica_data.BATCH, n) and data.dtype == np.float32
  np.testing.assert_allclose(
      np.concatenate([ica_data.guard(data), ica_data.guard(d0)]),
      golden[name + '_guard'], rtol=1e-9)
  # whitened: unit covariance; orthonormal start
  x = data.reshape(-1, n).astype(np.float64)
  assert np.abs(x.T @ x / x.shape[0] - np.eye(n)).max() < 1e-5
  assert np.abs(d0.astype(np.float64) @ d0.T - np.eye(n)).max() < 1e-5
  assert mixing.shape == (n, n)


@pytest.mark.parametrize('n', [64, 256])
@pytest.mark.parametrize('kappa', ica_data.KAPPAS)
def test_regenerated_code_inputs_match_the_fixture(golden, n, kappa):
  x, d = ica_data.code_inputs(n, kappa)
  tag = 'codes_n%d_k%.0e' % (n, kappa)
  np.testing.assert_allclose(
      np.concatenate([ica_data.guard(x), ica_data.guard(d)]),
      golden[tag + '_guard'], rtol=1e-9)
  assert np.linalg.cond(d.astype(np.float64)) == pytest.approx(kappa,
                                                               rel=1e-3)


def test_stored_reference_distances_stay_on_the_float64_trajectory(golden):
  keys = ['%s_step%d_dist' % (name, s) for name in ica_data.CASES
          for s in ica_data.HORIZONS[name]] + ['schedule_dist']
  for key in keys:
    assert float(golden[key]) <= 2e-6, key


def test_float64_statement_reproduces_the_stored_dictionaries(golden):
  n, nb, seed = ica_data.CASES['n64']
  data, _ = ica_data.batches(n, nb, seed)
  d0 = ica_data.init_dictionary(n, seed)
  for steps in ica_data.HORIZONS['n64']:
    truth = ica_data.truth_run(d0, data, {0: (ica_data.STEPSIZE, 1)}, steps)
    assert ica_data.rel(golden['n64_step%d' % steps], truth) <= 2e-6


def test_amari_index_of_the_truth_and_of_the_start():
  n, nb, seed = ica_data.RECOVERY
  _, mixing = ica_data.batches(n, 1, seed)
  perm = np.random.RandomState(0).permutation(n)
  scaled = mixing[perm] * np.linspace(0.5, 2, n)[:, None]
  assert ica_data.amari_index(scaled, mixing) < 1e-10
  start = ica_data.amari_index(ica_data.init_dictionary(n, seed), mixing)
  assert 0.25 < start < 0.35


def test_mat_inverse_rejects_bad_arguments_without_the_gpu():
  import vtc_hip
  lib = vtc_hip.load_library()
  p = ctypes.c_void_p(256)
  q = ctypes.c_void_p(1 << 20)
  big = 1 << 30
  assert lib.vtc_mat_inverse(None, 4, q, p, p, big, None) == \
      vtc_hip.ERR_INVALID_ARGUMENT
  assert lib.vtc_mat_inverse(p, 4, None, p, p, big, None) == \
      vtc_hip.ERR_INVALID_ARGUMENT
  assert lib.vtc_mat_inverse(p, 4, q, None, p, big, None) == \
      vtc_hip.ERR_INVALID_ARGUMENT
  assert lib.vtc_mat_inverse(p, 0, q, p, p, big, None) == \
      vtc_hip.ERR_INVALID_ARGUMENT
  assert lib.vtc_mat_inverse(p, -3, q, p, p, big, None) == \
      vtc_hip.ERR_INVALID_ARGUMENT
  # the output may not overlap the input
  assert lib.vtc_mat_inverse(p, 4, ctypes.c_void_p(256 + 16), p, p, big,
                             None) == vtc_hip.ERR_INVALID_ARGUMENT
  assert lib.vtc_mat_inverse(p, 257, q, p, p, big, None) == \
      vtc_hip.ERR_UNSUPPORTED
  assert b'256' in lib.vtc_last_error()
  need = lib.vtc_mat_inverse_workspace_bytes(64)
  assert need >= 64 * 64 * 8
  assert lib.vtc_mat_inverse(p, 64, q, p, p, need - 1, None) == \
      vtc_hip.ERR_WORKSPACE
  assert lib.vtc_mat_inverse(p, 64, q, p, None, need, None) == \
      vtc_hip.ERR_WORKSPACE
  assert lib.vtc_mat_inverse_workspace_bytes(256) >= 256 * 256 * 8
  assert lib.vtc_mat_inverse_workspace_bytes(33) >= 64 * 64 * 8


def _params(**extra):
  p = {'num_epochs': 1, 'dictionary_update_algorithm': 'ica_natural_gradient',
       'dict_update_param_schedule': {0: {'stepsize': 0.1, 'num_iters': 1}}}
  p.update(extra)
  return p


def test_train_dictionary_checks_its_parameters():
  from training import ica
  d = torch.eye(8)
  data = torch.zeros((2, 4, 8))
  with pytest.raises(AssertionError):
    ica.train_dictionary(data, d, _params(dict_update_param_schedule={
        1: {'stepsize': 0.1, 'num_iters': 1}}))
  with pytest.raises(AssertionError):
    ica.train_dictionary(data, torch.zeros((8, 6)), _params())
  with pytest.raises(AssertionError):
    ica.train_dictionary(data, d, _params(
        dictionary_update_algorithm='sc_steepest_descent'))


def test_train_dictionary_refuses_a_host_dictionary():
  import vtc_hip
  from training import ica
  with pytest.raises(vtc_hip.VtcHipError):
    ica.train_dictionary(torch.zeros((2, 4, 8)), torch.eye(8), _params())


def test_invertible_linear_refuses_host_tensors():
  import vtc_hip
  from analysis_transforms.fully_connected import invertible_linear
  with pytest.raises(vtc_hip.VtcHipError):
    invertible_linear.run(torch.zeros((4, 8)), torch.eye(8))
