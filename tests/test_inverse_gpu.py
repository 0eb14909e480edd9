"""The device matrix inverse (csrc/inverse.hip, vtc_hip.linalg.mat_inverse /
inverse) on the MI355X: accuracy against the float64 inverse over sizes and
condition numbers, pivoting, singular and non-finite inputs, the n > 256
library route, determinism and the bounds of its output."""
import ctypes

import numpy as np
import pytest
import torch

import fences
import ica_data

pytestmark = pytest.mark.gpu


def _lib():
  import vtc_hip
  return vtc_hip, vtc_hip.load_library()


@pytest.mark.parametrize('kappa', ica_data.KAPPAS)
@pytest.mark.parametrize('n', [1, 2, 3, 31, 64, 192, 255, 256])
def test_inverse_matches_float64(device, n, kappa):
  from vtc_hip import linalg
  a = ica_data.conditioned(n, kappa, 40 + n)
  x, status = linalg.mat_inverse(torch.from_numpy(a).to(device))
  assert status.tolist() == [1, -1]
  truth = np.linalg.inv(a.astype(np.float64))
  assert ica_data.rel(x.cpu().numpy(), truth) <= 1e-6


def test_inverse_of_a_permutation_is_exact(device):
  from vtc_hip import linalg
  n = 100
  p = np.eye(n, dtype=np.float32)[np.random.RandomState(3).permutation(n)]
  x = linalg.inverse(torch.from_numpy(p).to(device))
  assert np.array_equal(x.cpu().numpy(), p.T)


def test_inverse_pivots_past_a_zero_leading_entry(device):
  from vtc_hip import linalg
  a = np.random.RandomState(4).randn(64, 64).astype(np.float32)
  a[0, 0] = 0.0
  x, status = linalg.mat_inverse(torch.from_numpy(a).to(device))
  assert status.tolist() == [1, -1]
  assert ica_data.rel(x.cpu().numpy(),
                      np.linalg.inv(a.astype(np.float64))) <= 1e-6


def _singular_cases():
  rs = np.random.RandomState(5)
  dup = rs.randn(64, 64).astype(np.float32)
  dup[40] = dup[7]
  zero_col = rs.randn(64, 64).astype(np.float32)
  zero_col[:, 13] = 0.0
  nan = rs.randn(64, 64).astype(np.float32)
  nan[20, 30] = np.nan
  inf = rs.randn(64, 64).astype(np.float32)
  inf[3, 3] = np.inf
  return {'duplicated_row': dup, 'zero_column': zero_col, 'nan': nan,
          'inf': inf}


@pytest.mark.parametrize('kind', sorted(_singular_cases()))
def test_singular_and_nonfinite_inputs_are_reported(device, kind):
  from vtc_hip import linalg
  a = torch.from_numpy(_singular_cases()[kind]).to(device)
  _, status = linalg.mat_inverse(a)
  nonsingular, bad = status.tolist()
  assert nonsingular == 0
  if kind == 'zero_column':
    assert bad == 13
  if kind == 'duplicated_row':
    assert 0 <= bad < 64
  with pytest.raises(torch.linalg.LinAlgError):
    linalg.inverse(a)


def test_n257_is_unsupported_in_c_and_falls_back_in_python(device):
  from vtc_hip import linalg
  vtc_hip, lib = _lib()
  n = 257
  a = torch.from_numpy(ica_data.conditioned(n, 1e2, 9)).to(device)
  out = torch.empty_like(a)
  status = torch.empty(2, dtype=torch.int32, device=device)
  ws = vtc_hip.workspace(1 << 20, device)
  assert lib.vtc_mat_inverse(vtc_hip.ptr(a), n, vtc_hip.ptr(out),
                             vtc_hip.ptr(status), vtc_hip.ptr(ws), ws.numel(),
                             None) == vtc_hip.ERR_UNSUPPORTED
  x, status = linalg.mat_inverse(a)
  assert status.tolist() == [1, -1]
  truth = np.linalg.inv(a.cpu().numpy().astype(np.float64))
  assert ica_data.rel(x.cpu().numpy(), truth) <= 1e-6
  bad = a.clone()
  bad[:, 5] = 0
  with pytest.raises(torch.linalg.LinAlgError):
    linalg.inverse(bad)


def test_two_calls_are_bitwise_identical(device):
  from vtc_hip import linalg
  a = torch.from_numpy(ica_data.conditioned(256, 1e4, 11)).to(device)
  x1 = linalg.inverse(a)
  x2 = linalg.inverse(a)
  assert torch.equal(x1, x2)


@pytest.mark.parametrize('n', [5, 64, 256])
def test_canary_bytes_around_the_output_are_untouched(device, n):
  vtc_hip, lib = _lib()
  a = torch.from_numpy(ica_data.conditioned(n, 1e2, 12 + n)).to(device)
  pad = 1024
  canary = np.float32(-7.25)
  buf = torch.full((n * n + 2 * pad,), float(canary), dtype=torch.float32,
                   device=device)
  status = torch.empty(2, dtype=torch.int32, device=device)
  # the workspace at exactly the queried size, 0xFF-filled, between guards
  ws, ws_fence = fences.fenced_workspace(
      lib.vtc_mat_inverse_workspace_bytes(n), device)
  assert ws.numel() == lib.vtc_mat_inverse_workspace_bytes(n)
  out = buf[pad:pad + n * n]
  vtc_hip.check(lib.vtc_mat_inverse(
      vtc_hip.ptr(a), n, ctypes.c_void_p(out.data_ptr()), vtc_hip.ptr(status),
      vtc_hip.ptr(ws), ws.numel(), vtc_hip.current_stream(device)),
      'vtc_mat_inverse')
  ws_fence.assert_intact('vtc_mat_inverse workspace, n = %d' % n)
  host = buf.cpu().numpy()
  assert np.all(host[:pad] == canary) and np.all(host[pad + n * n:] == canary)
  assert status.tolist() == [1, -1]
  truth = np.linalg.inv(a.cpu().numpy().astype(np.float64))
  assert ica_data.rel(host[pad:pad + n * n].reshape(n, n), truth) <= 1e-6
