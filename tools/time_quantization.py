"""Times the scalar quantisers of include/vtc_quant.h (csrc/quantization.hip)
at the size of the experiment's Mod1 fit: b = 100 000 codes of s = 64
coefficients, Laplace-distributed with 90 % exact zeros, uniform codebooks of
bin width 5 over each column's range (utils.quantization.uniform_codebooks):

  vtc_quant_assign      HIP-event median of the raw C call (two launches),
                        lambda = 0 and lambda = 0.5, indices and dequantised
                        codes written
  vtc_quant_lloyd_step  the same for one step from the initial state (three
                        launches), lambda = 0.5, into a second state so that
                        every repetition does the same work
  scalar_lloyd          wall clock of a 20-step fit from Python, its one host
                        read included
  host                  the float64 numpy restatement of the same assign and
                        the same step (tests/quantization_data.py) on the host
                        of the same box, once each, for scale

Medians over REPS runs after WARMUP; minimum and maximum beside them.  The
device indices are checked against the host's before anything is timed.  There
is no threshold: this records what the run gives.

  timeout 900 python3 tools/time_quantization.py

profiles/quantization.txt holds this output and, under their own command, the
quantization_gap lines that tests/test_quantization_gpu.py prints.
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

import quantization_data as restatement  # noqa: E402
import vtc_hip  # noqa: E402
from utils import plotting  # noqa: E402
from utils import quantization  # noqa: E402

dev = torch.device('cuda:0')
WARMUP, REPS = 5, 50
B, S, WIDTH, SCALE, LAM = 100000, 64, 5.0, 20.0, 0.5


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
  rs = np.random.RandomState(100000)
  x = rs.laplace(scale=SCALE, size=(B, S))
  x[rs.rand(B, S) < 0.9] = 0.0
  x = x.astype(np.float32)
  codes = torch.from_numpy(x).to(dev)
  summary = plotting.code_summary(codes)
  books, k = quantization.uniform_codebooks(
      summary['min'].cpu().numpy(), summary['max'].cpu().numpy(), WIDTH)
  kmax = books.shape[1]
  print('codes %d x %d float32, Laplace scale %g, %.1f %% exact zeros; bin '
        'width %g: k = %d .. %d codewords per column, kmax = %d'
        % (B, S, SCALE, 100.0 * (x == 0).mean(), WIDTH, k.min(), k.max(), kmax))
  print('device: %s, torch %s' % (torch.cuda.get_device_name(0),
                                  torch.__version__))

  start, _ = restatement.initial_state(x, books, k)
  t0 = time.perf_counter()
  want0, _ = restatement.assign(x, books, k)
  host_assign0 = time.perf_counter() - t0
  t0 = time.perf_counter()
  want1, _ = restatement.assign(x, books, k, start['lengths'], LAM)
  host_assign1 = time.perf_counter() - t0
  t0 = time.perf_counter()
  host_state, _ = restatement.step(x, start, LAM, 1e-5, True)
  host_step = time.perf_counter() - t0

  values = torch.from_numpy(start['codebooks']).to(dev)
  k_dev = torch.from_numpy(start['k']).to(dev)
  lengths = torch.from_numpy(start['lengths']).to(dev)
  indices = torch.empty((B, S), dtype=torch.int32, device=dev)
  dequantized = torch.empty((B, S), dtype=torch.float32, device=dev)
  status = torch.empty(1, dtype=torch.int64, device=dev)

  def assign(lam):
    vtc_hip.check(lib.vtc_quant_assign(
        p(codes), B, S, p(values), p(lengths) if lam else None, p(k_dev), kmax,
        lam, p(indices), p(dequantized), p(status), stream), 'assign')

  for lam, want in ((0.0, want0), (LAM, want1)):
    assign(lam)
    torch.cuda.synchronize()
    assert np.array_equal(indices.cpu().numpy(), want), lam
  assert int(status) == 0

  names = [f[0] for f in vtc_hip.QuantState._fields_]
  state_in = {n: torch.from_numpy(np.ascontiguousarray(start[n])).to(dev)
              for n in names}
  state_out = {n: torch.empty_like(t) for n, t in state_in.items()}
  as_struct = lambda d: vtc_hip.QuantState(**{n: d[n].data_ptr()
                                              for n in names})
  s_in, s_out = as_struct(state_in), as_struct(state_out)
  ws_bytes = lib.vtc_quant_lloyd_step_workspace_bytes(B, S, kmax)
  ws = vtc_hip.workspace(ws_bytes, dev)

  def step():
    vtc_hip.check(lib.vtc_quant_lloyd_step(
        p(codes), B, S, kmax, LAM, 1e-5, 1, ctypes.byref(s_in),
        ctypes.byref(s_out), p(status), p(ws), ws.numel(), stream), 'step')

  step()
  torch.cuda.synchronize()
  for n in ('k', 'zero_index', 'counts', 'active', 'iterations'):
    assert np.array_equal(state_out[n].cpu().numpy(), host_state[n]), n
  gap = 0.0
  for n in ('codebooks', 'lengths', 'cost'):
    got, want = state_out[n].cpu().numpy(), host_state[n]
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), ok), n
    scale = np.maximum(np.abs(want[ok]), 1.0 if n == 'lengths' else 1e-300)
    gap = max(gap, float((np.abs(got[ok] - want[ok]) / scale).max()))
  print('one step against the host restatement: integers equal, largest '
        'relative gap of codebooks, lengths, cost %.2e' % gap)

  rows = [('vtc_quant_assign lambda = 0', device_ms(lambda: assign(0.0)),
           host_assign0),
          ('vtc_quant_assign lambda = %g' % LAM, device_ms(lambda: assign(LAM)),
           host_assign1),
          ('vtc_quant_lloyd_step lambda = %g' % LAM, device_ms(step), host_step)]
  print('workspace of the step: %.1f MiB' % (ws_bytes / 2.0**20))
  print('%-34s %10s %10s %10s %12s %8s' % ('call', 'median ms', 'min ms',
                                          'max ms', 'host numpy s', 'ratio'))
  for name, (median, low, high), host in rows:
    print('%-34s %10.3f %10.3f %10.3f %12.2f %8.0f'
          % (name, median, low, high, host, host * 1e3 / median))
  code_bytes = 4.0 * B * S
  print('assign lambda = 0: %.1f GB/s of codes read, %.2f G cell evaluations/s'
        % (code_bytes / rows[0][1][0] / 1e6,
           float(k.astype(np.float64).sum()) * B / rows[0][1][0] / 1e6))

  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fit = quantization.scalar_lloyd(codes, (books, k), lagrange_mult=LAM,
                                  max_iterations=20, epsilon=1e-5)
  wall = time.perf_counter() - t0
  print('scalar_lloyd, 20 steps enqueued, one read: %.1f ms wall; %d of %d '
        'columns converged, iterations %d .. %d, k %d .. %d'
        % (1e3 * wall, int(fit['converged'].sum()), S,
           fit['iterations'].min(), fit['iterations'].max(),
           int(fit['k'].min()), int(fit['k'].max())))


if __name__ == '__main__':
  main()
