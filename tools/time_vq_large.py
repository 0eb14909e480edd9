"""Times the large-codebook vector quantiser of include/vtc_vq_large.h
(csrc/vq_large.hip) at the size of the experiment's Mod2 / Mod3 fit, from the
start the experiment asks for: b = 100 000 vectors of d = 23 coefficients,
Laplace-distributed with about 90 % exact zeros and 60 % of the rows the zero
vector (tests/vq_data.vectors, the data of tools/time_vq.py), and the codebook
that initial_vector_codebook(num_bins = 100 000, max_codewords = 131 072)
gives: every distinct row.

  vtc_vq_large_assign      HIP-event median of the raw C call, lambda = 0 and
                           lambda = 0.5, indices and dequantised vectors written
  vtc_vq_large_lloyd_step  the same for one step from the initial state (six
                           launches), lambda = 0.5, into a second state so that
                           every repetition does the same work
  vector_lloyd             wall clock of a 20-step fit from Python with
                           max_codewords = 131 072, its one host read included,
                           twice in the same process
  old / new                at the capped start of today (4096 rows), one step
                           of vtc_vq_lloyd_step and one of
                           vtc_vq_large_lloyd_step side by side, their outputs
                           compared byte for byte, and the ratio of the medians
  Mod3_compute_RD_point    the experiment's call, vec_init_num_bins = 100000,
                           with vec_max_codewords = 131072, on 64-coefficient
                           codes whose tail is those vectors: wall clock

The first 1024 rows of both assignments are checked against the float64 numpy
restatement of tests/vq_data.py before anything is timed (the whole table of
distances would take 30 GB on the host).  Medians over REPS runs after WARMUP;
minimum and maximum beside them.  There is no threshold: this records what the
run gives.

  timeout 900 python3 tools/time_vq_large.py

profiles/vq_large.txt holds this output.
"""
import ctypes
import pathlib
import sys
import time

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
sys.path.insert(0, str(REPO / 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vq_data as restatement  # noqa: E402
import vtc_hip  # noqa: E402
from utils import vector_quantization as vq  # noqa: E402

dev = torch.device('cuda:0')
WARMUP, REPS = 3, 20
B, D, SCALE, LAM, NUM_BINS = 100000, 23, 0.7, 0.5, 100000
LARGE = vq.VQ_LARGE_MAX_CODEWORDS
CHECKED_ROWS = 1024


def device_ms(fn):
  for _ in range(WARMUP):
    fn()
  times = []
  for _ in range(REPS):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
  return float(np.median(times)), float(np.min(times)), float(np.max(times))


def initial_state(vectors, book_dev, limit):
  """The state vector_lloyd starts from, on the device, as numpy arrays."""
  kmax = book_dev.shape[0]
  indices = vq.vector_assign(vectors, book_dev, max_codewords=limit)
  counts = vq.vector_index_counts(indices, kmax, limit).cpu().numpy()
  book = book_dev.cpu().numpy()
  with np.errstate(divide='ignore'):
    lengths = -np.log2(counts / np.float64(counts.sum()))
  return {'codebook': book, 'lengths': lengths, 'counts': counts,
          'cost': np.zeros(3), 'k': np.array([kmax], np.int32),
          'zero_index': np.array([restatement.zero_point(book, kmax)],
                                 np.int32),
          'active': np.ones(1, np.int32), 'iterations': np.zeros(1, np.int32)}


class Step(object):
  """One step of `prefix`lloyd_step from `start` into a second state."""

  def __init__(self, lib, prefix, vectors, start):
    names = [f[0] for f in vtc_hip.VqState._fields_]
    self.state_in = {n: torch.from_numpy(np.ascontiguousarray(start[n])).to(dev)
                     for n in names}
    self.state_out = {n: torch.empty_like(t)
                      for n, t in self.state_in.items()}
    as_struct = lambda d: vtc_hip.VqState(**{n: d[n].data_ptr()
                                             for n in names})
    self.s_in, self.s_out = as_struct(self.state_in), as_struct(self.state_out)
    self.kmax = start['codebook'].shape[0]
    self.ws_bytes = getattr(lib, prefix + 'lloyd_step_workspace_bytes')(
        B, D, self.kmax)
    self.ws = vtc_hip.workspace(self.ws_bytes, dev)
    self.status = torch.empty(1, dtype=torch.int64, device=dev)
    self.entry, self.name = getattr(lib, prefix + 'lloyd_step'), prefix
    self.vectors = vectors

  def __call__(self):
    vtc_hip.check(self.entry(
        vtc_hip.ptr(self.vectors), B, D, self.kmax, LAM, 1e-5, 1,
        ctypes.byref(self.s_in), ctypes.byref(self.s_out),
        vtc_hip.ptr(self.status), vtc_hip.ptr(self.ws), self.ws.numel(),
        vtc_hip.current_stream(dev)), self.name + 'lloyd_step')


def main():
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  p = vtc_hip.ptr
  x = restatement.vectors(100000, B, D, scale=SCALE)
  vectors = torch.from_numpy(x).to(dev)
  book_dev = vq.initial_vector_codebook(vectors, NUM_BINS, max_codewords=LARGE)
  kmax = book_dev.shape[0]
  print('vectors %d x %d float32, Laplace scale %g, %.1f %% exact zeros, '
        '%.1f %% zero rows; initial_vector_codebook(num_bins = %d, '
        'max_codewords = %d): k = kmax = %d'
        % (B, D, SCALE, 100.0 * (x == 0).mean(),
           100.0 * (x == 0).all(1).mean(), NUM_BINS, LARGE, kmax))
  print('device: %s, torch %s' % (torch.cuda.get_device_name(0),
                                  torch.__version__))
  start = initial_state(vectors, book_dev, LARGE)
  book = start['codebook']

  k_dev = torch.from_numpy(start['k']).to(dev)
  lengths = torch.from_numpy(start['lengths']).to(dev)
  indices = torch.empty(B, dtype=torch.int32, device=dev)
  dequantized = torch.empty((B, D), dtype=torch.float32, device=dev)
  status = torch.empty(1, dtype=torch.int64, device=dev)

  def assign(lam):
    vtc_hip.check(lib.vtc_vq_large_assign(
        p(vectors), B, D, p(book_dev), p(lengths) if lam else None, p(k_dev),
        kmax, lam, p(indices), p(dequantized), p(status), stream), 'assign')

  for lam in (0.0, LAM):
    assign(lam)
    torch.cuda.synchronize()
    want, margin, _ = restatement.assign(x[:CHECKED_ROWS], book, kmax,
                                         start['lengths'], lam)
    assert np.array_equal(indices[:CHECKED_ROWS].cpu().numpy(), want), lam
    print('assign lambda = %g: the first %d rows equal the host restatement '
          '(margin %.2e)' % (lam, CHECKED_ROWS, margin))
  assert int(status) == 0

  step = Step(lib, 'vtc_vq_large_', vectors, start)
  step()
  torch.cuda.synchronize()
  print('one step, lambda = %g: k %d -> %d, zero cell %d rows, cost J %.6g'
        % (LAM, kmax, int(step.state_out['k']),
           int(step.state_out['counts'][int(step.state_out['zero_index'])]),
           float(step.state_out['cost'][0])))
  rows = [('vtc_vq_large_assign lambda = 0', device_ms(lambda: assign(0.0))),
          ('vtc_vq_large_assign lambda = %g' % LAM,
           device_ms(lambda: assign(LAM))),
          ('vtc_vq_large_lloyd_step lambda = %g' % LAM, device_ms(step))]
  print('workspace of the step at kmax = %d: %.1f MiB; at kmax = %d: %.1f MiB'
        % (kmax, step.ws_bytes / 2.0**20, LARGE,
           lib.vtc_vq_large_lloyd_step_workspace_bytes(B, D, LARGE) / 2.0**20))

  # the capped start of today: the old and the new step side by side
  small_book = vq.initial_vector_codebook(vectors, NUM_BINS)
  small_start = initial_state(vectors, small_book, vq.VQ_MAX_CODEWORDS)
  old = Step(lib, 'vtc_vq_', vectors, small_start)
  new = Step(lib, 'vtc_vq_large_', vectors, small_start)
  old()
  new()
  torch.cuda.synchronize()
  for n, t in old.state_out.items():
    assert np.array_equal(t.cpu().numpy().view(np.uint8),
                          new.state_out[n].cpu().numpy().view(np.uint8)), n
  print('capped start, k = kmax = %d: the two steps give the same bytes; '
        'workspace %.1f MiB (old) and %.1f MiB (new)'
        % (old.kmax, old.ws_bytes / 2.0**20, new.ws_bytes / 2.0**20))
  old_ms, new_ms = device_ms(old), device_ms(new)
  rows += [('vtc_vq_lloyd_step, k = %d' % old.kmax, old_ms),
           ('vtc_vq_large_lloyd_step, k = %d' % old.kmax, new_ms)]
  print('%-40s %10s %10s %10s' % ('call', 'median ms', 'min ms', 'max ms'))
  for name, (median, low, high) in rows:
    print('%-40s %10.3f %10.3f %10.3f' % (name, median, low, high))
  print('new / old step at k = %d: %.3f' % (old.kmax, new_ms[0] / old_ms[0]))
  print('assign lambda = 0: %.2f G cell evaluations/s'
        % (float(kmax) * B / rows[0][1][0] / 1e6))

  # twice: the first call also loads the code objects of the few torch
  # operators that vector_lloyd uses for its plumbing, once per process
  for label in ('first call', 'second call'):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = vq.vector_lloyd(vectors, book_dev, lagrange_mult=LAM,
                          max_iterations=20, epsilon=1e-5, max_codewords=LARGE)
    wall = time.perf_counter() - t0
    print('vector_lloyd, 20 steps enqueued, one read, %s: %.1f ms wall; '
          'converged %s, iterations %d, k %d of kmax %d'
          % (label, 1e3 * wall, fit['converged'], fit['iterations'],
             int(fit['k']), fit['codebook'].shape[0]))

  # the experiment's call: 41 scalar coefficients and the 23 of the tail
  rs = np.random.RandomState(7)
  codes = np.zeros((B, 64), np.float32)
  codes[:, restatement.VEC_CLUST] = x
  scalars = rs.laplace(size=(B, len(restatement.SCAL_CLUSTS))) * 20.0
  scalars[rs.rand(*scalars.shape) < 0.5] = 0.0
  codes[:, restatement.SCAL_CLUSTS] = scalars
  dictionary = rs.randn(64, 64)
  dictionary /= np.linalg.norm(dictionary, axis=1, keepdims=True)
  codes_dev = torch.from_numpy(codes).to(dev)
  dictionary_dev = torch.from_numpy(dictionary.astype(np.float32)).to(dev)
  patches_dev = codes_dev @ dictionary_dev + torch.from_numpy(
      rs.randn(B, 64).astype(np.float32)).to(dev)
  for label in ('first call', 'second call'):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = vq.Mod3_compute_RD_point(
        codes_dev, patches_dev, dictionary_dev, restatement.SCAL_CLUSTS,
        restatement.VEC_CLUST, scal_quant_multiplier=2.0,
        scal_binwidths=[restatement.SCAL_WIDTH] * len(restatement.SCAL_CLUSTS),
        vec_quant_multiplier=LAM, vec_init_num_bins=NUM_BINS,
        vec_max_codewords=LARGE)
    wall = time.perf_counter() - t0
    print('Mod3_compute_RD_point(vec_init_num_bins = %d, vec_max_codewords = '
          '%d), %s: %.1f ms wall; rate %.4f bits/pixel, pSNR %.2f dB, vector '
          'codebook k %d of kmax %d'
          % (NUM_BINS, LARGE, label, 1e3 * wall, out[0], out[1]['pSNR'],
             int(out[3]['k']), out[3]['codebook'].shape[0]))


if __name__ == '__main__':
  main()
