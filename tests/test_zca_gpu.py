"""ZCA whitening, PCA and their primitives on the MI355X (csrc/zca.hip):
the Jacobi eigen-solver, the float64 covariance, whiten_ZCA / unwhiten_ZCA /
training.pca.train_dictionary against the reference (tests/golden/zca.npz)
and the float64 statement of tests/zca_data.py, the library fallbacks and a
large batch run twice."""
import warnings

import numpy as np
import pytest
import torch

import zca_data
from helpers import load

pytestmark = pytest.mark.gpu

K = zca_data.STORED_ROWS


@pytest.fixture(scope='module')
def golden():
  return load('zca')


def _lib():
  import vtc_hip
  return vtc_hip, vtc_hip.load_library()


# ---- eigen-solver -------------------------------------------------------
def _random_orthogonal(rs, n):
  q, r = np.linalg.qr(rs.randn(n, n))
  return q * np.sign(np.diag(r))[None, :]


def _matrix(kind, n, seed):
  rs = np.random.RandomState(seed)
  if kind == 'symmetric':      # negative eigenvalues
    a = rs.randn(n, n)
    return (a + a.T) / 2
  if kind == 'psd_zeros':      # exact zero eigenvalues (rank n // 2)
    b = rs.randn(n, max(n // 2, 1))
    return b @ b.T
  if kind == 'identity_rank1':  # n - 1 fold repeated eigenvalue
    v = rs.randn(n, 1)
    return np.eye(n) + v @ v.T
  q = _random_orthogonal(rs, n)
  if kind == 'clusters':        # groups of 4 within 1e-9 relative
    w = np.repeat(rs.rand((n + 3) // 4) + 1, 4)[:n]
    w = w * (1 + 1e-9 * rs.rand(n))
  elif kind == 'diagonal':
    return np.diag(rs.randn(n))
  else:                         # covariance-like, 4 decades
    w = np.logspace(0, -4, n)
  return (q * w[None, :]) @ q.T


KINDS = ['symmetric', 'psd_zeros', 'identity_rank1', 'clusters', 'diagonal',
         'covariance']


@pytest.mark.parametrize('n', [1, 2, 3, 17, 64, 100, 192, 256])
@pytest.mark.parametrize('kind', KINDS)
def test_sym_eig(device, kind, n):
  from vtc_hip import linalg
  a = _matrix(kind, n, 100 + n)
  w, u, status = linalg.sym_eig(torch.from_numpy(a).to(device))
  converged, sweeps = status.tolist()
  assert converged == 1 and 0 <= sweeps <= linalg.JACOBI_MAX_SWEEPS
  w = w.cpu().numpy()
  u32 = u.cpu().numpy()
  v = u32.astype(np.float64)
  norm2 = max(np.abs(np.linalg.eigvalsh(a)).max(), 1e-300)
  assert np.linalg.norm(a @ v - v * w[None, :]) <= 2e-6 * np.linalg.norm(a)
  assert np.abs(v.T @ v - np.eye(n)).max() <= 2e-6
  ref = np.linalg.eigvalsh(a)[::-1]
  assert np.abs(w - ref).max() <= 1e-6 * norm2
  assert np.all(np.diff(w) <= 0)
  lead = np.argmax(np.abs(u32), axis=0)
  assert np.all(u32[lead, np.arange(n)] > 0)


def test_sym_eig_reports_no_convergence(device):
  from vtc_hip import linalg
  a = _matrix('symmetric', 64, 7)
  _, _, status = linalg.sym_eig(torch.from_numpy(a).to(device), max_sweeps=1)
  assert status.tolist() == [0, 1]


def test_sym_eig_rejects_n_above_256(device):
  vtc_hip, lib = _lib()
  a = torch.zeros((257, 257), dtype=torch.float64, device=device)
  w = torch.empty(257, dtype=torch.float64, device=device)
  u = torch.empty((257, 257), dtype=torch.float32, device=device)
  st = torch.empty(2, dtype=torch.int32, device=device)
  rc = lib.vtc_sym_eig(vtc_hip.ptr(a), 257, 10, vtc_hip.ptr(w),
                       vtc_hip.ptr(u), vtc_hip.ptr(st), None, 0, None)
  assert rc == vtc_hip.ERR_UNSUPPORTED


# ---- covariance --------------------------------------------------------------
COV_SHAPES = [(1, 1), (1, 64), (31, 64), (31, 192), (4097, 1), (4097, 64),
              (4097, 192), (4097, 256), (1000003, 1), (1000003, 64),
              (1000003, 256)]


@pytest.mark.parametrize('center', [True, False])
@pytest.mark.parametrize('rows,n', COV_SHAPES)
def test_column_covariance(device, rows, n, center):
  from vtc_hip import linalg
  g = torch.Generator().manual_seed(rows * 7 + n)
  x = (0.5 + 0.05 * torch.randn(rows, n, generator=g)).to(torch.float32)
  cov, means, grand = linalg.column_covariance(x.to(device), center)
  x64 = x.to(torch.float64)
  mu = x64.mean(0)
  xc = x64 - mu if center else x64
  truth = (xc.t() @ xc) / rows
  cov = cov.cpu()
  assert torch.equal(cov, cov.t())
  # D = 1 centred: the truth is exactly zero, and so must the result be
  assert float((cov - truth).norm()) <= 1e-9 * float(truth.norm())
  assert float((means.cpu() - mu).abs().max()) <= 1e-12
  assert abs(float(grand.cpu()[0]) - float(mu.mean())) <= 1e-12


# ---- whiten_ZCA / unwhiten_ZCA / pca ----------------------------------------
def _ref_params(golden, name):
  return {'PCA_basis': golden[name + '_basis'],
          'PCA_axis_variances': golden[name + '_variances'],
          'subtracted_mean': golden[name + '_mean']}


def _gap_ok(w, i, tol=1e-3):
  gap = np.abs(np.diff(w)) / w[0]
  return (i == 0 or gap[i - 1] >= tol) and (i == len(w) - 1 or gap[i] >= tol)


@pytest.mark.parametrize('name', sorted(zca_data.CASES))
def test_whiten_zca_estimating(device, golden, name):
  from utils import image_processing as ip
  est, _ = zca_data.case_data(name)
  white, params = ip.whiten_ZCA(torch.from_numpy(est).to(device))
  assert white.is_cuda and white.dtype == torch.float32
  white = white.cpu().numpy()
  t_white, t_params = zca_data.truth_estimate(est)
  assert zca_data.rel(white, t_white) <= 2e-6
  assert zca_data.rel(white[:K], golden[name + '_white']) <= 3e-5
  lam = t_params['PCA_axis_variances']
  w = params['PCA_axis_variances'].cpu().numpy()
  assert np.abs(w - lam).max() <= 1e-6 * lam[0]
  assert np.abs(w - golden[name + '_variances']).max() <= 1e-6 * lam[0]
  assert abs(float(params['subtracted_mean'].cpu()) -
             float(golden[name + '_mean'])) <= 1e-6
  u = params['PCA_basis'].cpu().numpy()
  u_ref = golden[name + '_basis']
  for i in range(u.shape[1]):
    if _gap_ok(lam, i):
      assert abs(np.dot(u[:, i], u_ref[:, i])) >= 1 - 1e-5
  # the whole W is unique: compare it everywhere
  wm = (u.astype(np.float64) / (np.sqrt(w.astype(np.float64)) + 1e-4)) @ \
      u.T.astype(np.float64)
  t_u = t_params['PCA_basis']
  t_wm = (t_u / (np.sqrt(lam) + 1e-4)) @ t_u.T
  assert zca_data.rel(wm, t_wm) <= 2e-6


@pytest.mark.parametrize('name', sorted(zca_data.CASES))
def test_whiten_and_unwhiten_with_reference_parameters(device, golden, name):
  from utils import image_processing as ip
  _, held = zca_data.case_data(name)
  params = _ref_params(golden, name)
  pre = ip.whiten_ZCA(torch.from_numpy(held).to(device), params).cpu().numpy()
  assert zca_data.rel(pre[:K], golden[name + '_pre']) <= 5e-6
  assert zca_data.rel(pre, zca_data.truth_whiten(held, params)) <= 2e-6
  back = ip.unwhiten_ZCA(torch.from_numpy(golden[name + '_pre']).to(device),
                         params).cpu().numpy()
  assert zca_data.rel(back, golden[name + '_unwhite']) <= 5e-6


def test_round_trip_keeps_the_reference_asymmetry(device):
  from utils import image_processing as ip
  est, _ = zca_data.case_data('n64')
  x = torch.from_numpy(est).to(device)
  white, params = ip.whiten_ZCA(x)
  back = ip.unwhiten_ZCA(white, params).cpu().numpy()
  assert 1e-3 < zca_data.rel(back, est) < 1e-2
  # with the scalar mean on both sides the round trip is exact to f32 noise
  white2 = ip.whiten_ZCA(x, params)
  back2 = ip.unwhiten_ZCA(white2, params).cpu().numpy()
  assert zca_data.rel(back2, est) < 1e-5


def test_whiten_zca_accepts_uint8(device):
  from utils import image_processing as ip
  est, _ = zca_data.case_data('n64')
  q = np.round(est * 255).astype(np.uint8)
  white, _ = ip.whiten_ZCA(torch.from_numpy(q).to(device))
  t_white, _ = zca_data.truth_estimate(q.astype(np.float32))
  assert zca_data.rel(white.cpu().numpy(), t_white) <= 2e-6


def test_whiten_zca_needs_ten_samples_per_component(device):
  from utils import image_processing as ip
  x = torch.rand(639, 64, device=device)
  with pytest.raises(RuntimeError):
    ip.whiten_ZCA(x)


def test_pca_train_dictionary(device, golden):
  from training import pca
  x = zca_data.pca_data()
  d = pca.train_dictionary(torch.from_numpy(x).to(device))
  assert d.is_cuda and d.shape == (64, 64) and d.dtype == torch.float32
  d = d.cpu().numpy()
  x64 = x.astype(np.float64)
  lam, t_u = zca_data.eigh_desc(x64.T @ x64 / x.shape[0])
  ref = golden['pca_dictionary']
  for i in range(64):
    if _gap_ok(lam, i):
      assert abs(np.dot(d[i], ref[i])) >= 1 - 1e-5
      assert abs(np.dot(d[i], t_u[:, i])) >= 1 - 1e-6
  assert np.abs(d @ d.T - np.eye(64)).max() <= 2e-6
  lead = np.argmax(np.abs(d), axis=1)
  assert np.all(d[np.arange(64), lead] > 0)


def test_pca_asserts_mean_zero(device):
  from training import pca
  est, _ = zca_data.case_data('n64')
  with pytest.raises(AssertionError):
    pca.train_dictionary(torch.from_numpy(est).to(device))


def test_pca_more_dimensions_than_samples(device):
  from training import pca
  rs = np.random.RandomState(3)
  x = rs.randn(40, 300).astype(np.float32)
  x -= x.mean(axis=0)
  d = pca.train_dictionary(torch.from_numpy(x).to(device)).cpu().numpy()
  assert d.shape == (40, 300)
  x64 = x.astype(np.float64)
  _, s, vt = np.linalg.svd(x64, full_matrices=False)
  for i in range(39):   # the last singular value is ~0 (centred data)
    if s[i] - s[i + 1] > 1e-3 * s[0] and (i == 0 or
                                          s[i - 1] - s[i] > 1e-3 * s[0]):
      assert abs(np.dot(d[i], vt[i])) >= 1 - 1e-5


# ---- fallbacks -------------------------------------------------------------
def _correlated(rows, n, seed):
  rs = np.random.RandomState(seed)
  q = _random_orthogonal(rs, n)
  scale = np.logspace(0, -1.5, n)
  return (0.5 + 0.1 * (rs.randn(rows, n) * scale[None, :]) @ q.T).astype(
      np.float32)


def test_fallback_above_256(device):
  from utils import image_processing as ip
  from training import pca
  x = _correlated(3200, 300, 5)
  white, params = ip.whiten_ZCA(torch.from_numpy(x).to(device))
  t_white, t_params = zca_data.truth_estimate(x)
  assert zca_data.rel(white.cpu().numpy(), t_white) <= 2e-6
  lam = t_params['PCA_axis_variances']
  w = params['PCA_axis_variances'].cpu().numpy()
  assert np.abs(w - lam).max() <= 1e-6 * lam[0]
  xc = (x - x.mean(axis=0, dtype=np.float64)).astype(np.float32)
  d = pca.train_dictionary(torch.from_numpy(xc).to(device)).cpu().numpy()
  assert d.shape == (300, 300)
  assert np.abs(d @ d.T - np.eye(300)).max() <= 2e-6


def test_fallback_when_jacobi_does_not_converge(device, monkeypatch):
  from utils import image_processing as ip
  from vtc_hip import linalg
  est, _ = zca_data.case_data('n64')
  monkeypatch.setattr(linalg, 'JACOBI_MAX_SWEEPS', 1)
  with pytest.warns(RuntimeWarning, match='did not converge'):
    white, params = ip.whiten_ZCA(torch.from_numpy(est).to(device))
  t_white, t_params = zca_data.truth_estimate(est)
  assert zca_data.rel(white.cpu().numpy(), t_white) <= 2e-6
  u = params['PCA_basis'].cpu().numpy()
  lead = np.argmax(np.abs(u), axis=0)
  assert np.all(u[lead, np.arange(64)] > 0)


# ---- large batch: bitwise repeatable ----------------------------------------
def test_large_batch_bitwise(device):
  from utils import image_processing as ip
  rows, n = 1 << 20, 64
  x = torch.from_numpy(_correlated(rows, n, 9)).to(device)
  runs = []
  for _ in range(2):
    white, params = ip.whiten_ZCA(x)
    pre = ip.whiten_ZCA(x, params)
    back = ip.unwhiten_ZCA(pre, params)
    torch.cuda.synchronize()
    runs.append([white, params['PCA_basis'], params['PCA_axis_variances'],
                 pre, back])
  for a, b in zip(*runs):
    assert torch.equal(a, b)
  # a 4096-row sample against the float64 statement over all rows
  sample = np.random.RandomState(1).choice(rows, 4096, replace=False)
  x64 = x.cpu().numpy().astype(np.float64)
  mu = x64.mean(axis=0)
  x64 -= mu
  lam, t_u = zca_data.eigh_desc(x64.T @ x64 / rows)
  t_params = {'PCA_basis': t_u, 'PCA_axis_variances': lam,
              'subtracted_mean': mu.mean()}
  t_wm = (t_u / (np.sqrt(lam) + 1e-4)) @ t_u.T
  t_white = x64[sample] @ t_wm + mu.mean()
  white, u, w, pre, back = [t.cpu().numpy() for t in runs[0]]
  assert zca_data.rel(white[sample], t_white) <= 2e-6
  assert np.abs(w - lam).max() <= 1e-6 * lam[0]
  xs = x64[sample] + mu
  params = {'PCA_basis': u, 'PCA_axis_variances': w,
            'subtracted_mean': np.float32(mu.mean())}
  assert zca_data.rel(pre[sample],
                      zca_data.truth_whiten(xs.astype(np.float32),
                                            params)) <= 2e-6
  assert zca_data.rel(back[sample],
                      zca_data.truth_unwhiten(pre[sample], params)) <= 2e-6
