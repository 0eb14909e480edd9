"""Times the vector quantiser of include/vtc_vq.h (csrc/vq.hip) at the size of
the experiment's Mod2 / Mod3 fit: b = 100 000 vectors of d = 23 coefficients,
Laplace-distributed with about 90 % exact zeros and 60 % of the rows the zero
vector (tests/vq_data.vectors), from the codebook that
utils.vector_quantization.initial_vector_codebook gives for the experiment's
vec_init_num_bins = 100 000:

  vtc_vq_assign      HIP-event median of the raw C call (two launches),
                     lambda = 0 and lambda = 0.5, indices and dequantised
                     vectors written
  vtc_vq_lloyd_step  the same for one step from the initial state (five
                     launches), lambda = 0.5, into a second state so that every
                     repetition does the same work
  vector_lloyd       wall clock of a 20-step fit from Python, its one host
                     read included, twice in the same process
  host               the float64 numpy restatement of the same assign and the
                     same step (tests/vq_data.py) on the host of the same box,
                     once each, for scale

Medians over REPS runs after WARMUP; minimum and maximum beside them.  The
device indices are checked against the host's before anything is timed.  There
is no threshold: this records what the run gives, and the workspace size.

  timeout 900 python3 tools/time_vq.py

profiles/vq.txt holds this output and, under their own command, the vq_gap
lines that tests/test_vq_gpu.py prints.
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
WARMUP, REPS = 5, 50
B, D, SCALE, LAM, NUM_BINS = 100000, 23, 0.7, 0.5, 100000


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


def main():
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  p = vtc_hip.ptr
  x = restatement.vectors(100000, B, D, scale=SCALE)
  vectors = torch.from_numpy(x).to(dev)
  book_dev = vq.initial_vector_codebook(vectors, NUM_BINS)
  book = book_dev.cpu().numpy()
  assert np.array_equal(book, restatement.initial_codebook(x, NUM_BINS))
  kmax = book.shape[0]
  print('vectors %d x %d float32, Laplace scale %g, %.1f %% exact zeros, '
        '%.1f %% zero rows; initial_vector_codebook(num_bins = %d): k = kmax '
        '= %d' % (B, D, SCALE, 100.0 * (x == 0).mean(),
                  100.0 * (x == 0).all(1).mean(), NUM_BINS, kmax))
  print('device: %s, torch %s' % (torch.cuda.get_device_name(0),
                                  torch.__version__))

  t0 = time.perf_counter()
  want0, _, _ = restatement.assign(x, book, kmax)
  host_assign0 = time.perf_counter() - t0
  counts = restatement.index_counts(want0, kmax)   # restatement.initial_state
  with np.errstate(divide='ignore'):
    first_lengths = -np.log2(counts / np.float64(counts.sum()))
  start = {'codebook': book.copy(), 'lengths': first_lengths, 'counts': counts,
           'cost': np.zeros(3), 'k': np.array([kmax], np.int32),
           'zero_index': np.array([restatement.zero_point(book, kmax)],
                                  np.int32),
           'active': np.ones(1, np.int32), 'iterations': np.zeros(1, np.int32)}
  t0 = time.perf_counter()
  want1, _, _ = restatement.assign(x, book, kmax, start['lengths'], LAM)
  host_assign1 = time.perf_counter() - t0
  t0 = time.perf_counter()
  host_state, facts = restatement.step(x, start, LAM, 1e-5, True)
  host_step = time.perf_counter() - t0
  print('host step: k %d -> %d, %d rows moved off their nearest codeword, '
        'zero cell %.1f %% of the rows, margin %.2e'
        % (kmax, int(host_state['k'][0]), facts['moved'],
           100.0 * facts['zero_share'], facts['margin']))

  k_dev = torch.from_numpy(start['k']).to(dev)
  lengths = torch.from_numpy(start['lengths']).to(dev)
  indices = torch.empty(B, dtype=torch.int32, device=dev)
  dequantized = torch.empty((B, D), dtype=torch.float32, device=dev)
  status = torch.empty(1, dtype=torch.int64, device=dev)

  def assign(lam):
    vtc_hip.check(lib.vtc_vq_assign(
        p(vectors), B, D, p(book_dev), p(lengths) if lam else None, p(k_dev),
        kmax, lam, p(indices), p(dequantized), p(status), stream), 'assign')

  for lam, want in ((0.0, want0), (LAM, want1)):
    assign(lam)
    torch.cuda.synchronize()
    assert np.array_equal(indices.cpu().numpy(), want), lam
  assert int(status) == 0

  names = [f[0] for f in vtc_hip.VqState._fields_]
  state_in = {n: torch.from_numpy(np.ascontiguousarray(start[n])).to(dev)
              for n in names}
  state_out = {n: torch.empty_like(t) for n, t in state_in.items()}
  as_struct = lambda d: vtc_hip.VqState(**{n: d[n].data_ptr() for n in names})
  s_in, s_out = as_struct(state_in), as_struct(state_out)
  ws_bytes = lib.vtc_vq_lloyd_step_workspace_bytes(B, D, kmax)
  ws = vtc_hip.workspace(ws_bytes, dev)

  def step():
    vtc_hip.check(lib.vtc_vq_lloyd_step(
        p(vectors), B, D, kmax, LAM, 1e-5, 1, ctypes.byref(s_in),
        ctypes.byref(s_out), p(status), p(ws), ws.numel(), stream), 'step')

  step()
  torch.cuda.synchronize()
  for n in ('k', 'zero_index', 'counts', 'active', 'iterations'):
    assert np.array_equal(state_out[n].cpu().numpy(), host_state[n]), n
  gap = 0.0
  for n in ('codebook', 'lengths', 'cost'):
    got, want = state_out[n].cpu().numpy(), host_state[n]
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), ok), n
    scale = np.maximum(np.abs(want[ok]), 1.0 if n == 'lengths' else 1e-300)
    gap = max(gap, float((np.abs(got[ok] - want[ok]) / scale).max()))
  print('one step against the host restatement: integers equal, largest '
        'relative gap of codebook, lengths, cost %.2e' % gap)

  rows = [('vtc_vq_assign lambda = 0', device_ms(lambda: assign(0.0)),
           host_assign0),
          ('vtc_vq_assign lambda = %g' % LAM, device_ms(lambda: assign(LAM)),
           host_assign1),
          ('vtc_vq_lloyd_step lambda = %g' % LAM, device_ms(step), host_step)]
  print('workspace of the step at kmax = %d: %.1f MiB; at kmax = 4096: %.1f '
        'MiB' % (kmax, ws_bytes / 2.0**20,
                 lib.vtc_vq_lloyd_step_workspace_bytes(B, D, 4096) / 2.0**20))
  print('%-34s %10s %10s %10s %12s %8s' % ('call', 'median ms', 'min ms',
                                          'max ms', 'host numpy s', 'ratio'))
  for name, (median, low, high), host in rows:
    print('%-34s %10.3f %10.3f %10.3f %12.2f %8.0f'
          % (name, median, low, high, host, host * 1e3 / median))
  print('assign lambda = 0: %.2f G cell evaluations/s, %.1f G float64 '
        'operations/s (3 per component, 24 padded components)'
        % (float(kmax) * B / rows[0][1][0] / 1e6,
           72.0 * kmax * B / rows[0][1][0] / 1e6))

  # twice: the first call also loads the code objects of the few torch
  # operators that vector_lloyd uses for its plumbing, once per process
  for label in ('first call', 'second call'):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fit = vq.vector_lloyd(vectors, book_dev, lagrange_mult=LAM,
                          max_iterations=20, epsilon=1e-5)
    wall = time.perf_counter() - t0
    print('vector_lloyd, 20 steps enqueued, one read, %s: %.1f ms wall; '
          'converged %s, iterations %d, k %d'
          % (label, 1e3 * wall, fit['converged'], fit['iterations'],
             int(fit['k'])))


if __name__ == '__main__':
  main()
