"""ZCA / PCA without a GPU: the fixture's inputs regenerate, the float64
statement the GPU tests gate against reproduces the reference's outputs, and
the new C entry points reject bad arguments before any HIP call."""
import numpy as np
import pytest

import zca_data
from helpers import load


@pytest.fixture(scope='module')
def golden():
  return load('zca')


@pytest.mark.parametrize('name', sorted(zca_data.CASES))
def test_regenerated_inputs_match_the_fixture(golden, name):
  est, held = zca_data.case_data(name)
  n, _, d_est, d_test, _ = zca_data.CASES[name]
  assert est.shape == (d_est, n) and held.shape == (d_test, n)
  assert d_est >= 10 * n
  np.testing.assert_allclose(zca_data.guard(est), golden[name + '_guard_est'],
                             rtol=1e-9)
  np.testing.assert_allclose(zca_data.guard(held),
                             golden[name + '_guard_held'], rtol=1e-9)
  np.testing.assert_allclose(est[:2], golden[name + '_head_est'], rtol=1e-6,
                             atol=1e-7)
  np.testing.assert_allclose(held[:2], golden[name + '_head_held'],
                             rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize('name', sorted(zca_data.CASES))
def test_float64_statement_reproduces_the_reference(golden, name):
  """The reference is float32 (measured distance to this statement: 6-7e-6
  estimating, <= 4e-7 with its own parameters); the statement's centring
  asymmetry is the reference's."""
  est, held = zca_data.case_data(name)
  k = zca_data.STORED_ROWS
  params = {'PCA_basis': golden[name + '_basis'],
            'PCA_axis_variances': golden[name + '_variances'],
            'subtracted_mean': golden[name + '_mean']}
  white, t_params = zca_data.truth_estimate(est)
  assert zca_data.rel(golden[name + '_white'], white[:k]) < 2e-5
  lam = t_params['PCA_axis_variances']
  assert np.abs(params['PCA_axis_variances'] - lam).max() < 1e-7 * lam[0]
  assert abs(float(params['subtracted_mean']) -
             t_params['subtracted_mean']) < 1e-6
  assert zca_data.rel(golden[name + '_pre'],
                      zca_data.truth_whiten(held[:k], params)) < 2e-6
  assert zca_data.rel(golden[name + '_unwhite'],
                      zca_data.truth_unwhiten(golden[name + '_pre'],
                                              params)) < 1e-6
  # the asymmetry: unwhitening an estimating call does not give x back
  back = zca_data.truth_unwhiten(white, t_params)
  assert 1e-3 < zca_data.rel(back, est) < 3e-2


def test_pca_fixture_is_the_covariance_eigenbasis(golden):
  x = zca_data.pca_data().astype(np.float64)
  w, u = zca_data.eigh_desc(x.T @ x / x.shape[0])
  ref = golden['pca_dictionary']
  gap = np.abs(np.diff(w)) / w[0]
  for i in range(ref.shape[0]):
    if (i == 0 or gap[i - 1] >= 1e-3) and (i == len(gap) or gap[i] >= 1e-3):
      assert abs(np.dot(ref[i], u[:, i])) > 1 - 1e-4


def test_zca_entry_points_reject_bad_arguments_without_the_gpu():
  import vtc_hip
  lib = vtc_hip.load_library()
  checks = [
      lib.vtc_column_covariance(None, 4, 4, 1, None, None, None, None, 0,
                                None),
      lib.vtc_column_covariance(vtc_hip.ctypes.c_void_p(256), 0, 4, 1, None,
                                None, vtc_hip.ctypes.c_void_p(256), None, 0,
                                None),
      lib.vtc_sym_eig(None, 4, 10, None, None, None, None, 0, None),
      lib.vtc_sym_eig(vtc_hip.ctypes.c_void_p(256), 0, 10,
                      vtc_hip.ctypes.c_void_p(256),
                      vtc_hip.ctypes.c_void_p(256),
                      vtc_hip.ctypes.c_void_p(256), None, 0, None),
      lib.vtc_zca_matrices(None, None, 4, 1e-4, None, None, None),
      lib.vtc_row_transform(None, 4, 4, None, None, 0.0, None, None),
      lib.vtc_row_transform(vtc_hip.ctypes.c_void_p(256), 4, 0,
                            vtc_hip.ctypes.c_void_p(256),
                            vtc_hip.ctypes.c_void_p(256), 0.0,
                            vtc_hip.ctypes.c_void_p(256), None),
  ]
  assert checks == [vtc_hip.ERR_INVALID_ARGUMENT] * len(checks)
  # n > 256 is unsupported by the Jacobi solver, still before any HIP call
  p = vtc_hip.ctypes.c_void_p(256)
  assert lib.vtc_sym_eig(p, 257, 10, p, p, p, p, 1 << 30, None) == \
      vtc_hip.ERR_UNSUPPORTED
  assert b'256' in lib.vtc_last_error()
  # too small a workspace is refused
  assert lib.vtc_sym_eig(p, 64, 10, p, p, p, p, 16, None) == \
      vtc_hip.ERR_WORKSPACE
  assert lib.vtc_column_covariance(p, 1000, 64, 1, None, None, p, p, 16,
                                   None) == vtc_hip.ERR_WORKSPACE


def test_zca_workspace_queries_are_host_only():
  import vtc_hip
  lib = vtc_hip.load_library()
  assert lib.vtc_sym_eig_workspace_bytes(256) >= 2 * 256 * 256 * 8
  assert lib.vtc_sym_eig_workspace_bytes(17) >= 2 * 18 * 18 * 8
  assert lib.vtc_column_covariance_workspace_bytes(1 << 20, 256) >= 256 * 8
