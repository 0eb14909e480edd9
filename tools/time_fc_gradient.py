"""vtc_fc_dict_gradient per route (VTC_FC_GRAD=f32|b3|b3x1): HIP-event times
over the batch sizes of the cut-over sweep, and the relative error of grad_sum
against float64 where the float64 product is cheap (b <= 8192).

  python3 tools/time_fc_gradient.py [reps] >> profiles/fc_gradient_b3.txt

A route wins a shape when the difference of medians is at least twice the
larger min-max range of the two arms.
"""
import os
import pathlib
import sys

import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
import vtc_hip

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 15
ROUTES = ('f32', 'b3', 'b3x1')
dev = torch.device('cuda:0')
lib = vtc_hip.load_library()


def problem(b, n, s):
  g = torch.Generator(device=dev).manual_seed(b + n + s)
  X = 0.1 * torch.randn(b, n, device=dev, generator=g)
  D = torch.randn(s, n, device=dev, generator=g)
  D /= D.norm(dim=1, keepdim=True)
  C = 0.05 * torch.randn(b, s, device=dev, generator=g) * (
      torch.rand(b, s, device=dev, generator=g) < 0.2)
  return X, D, C


def run(route, X, D, C, ws, out, reps):
  os.environ['VTC_FC_GRAD'] = route
  b, n = X.shape
  s = D.shape[0]
  stream = vtc_hip.current_stream(dev)
  call = lambda: vtc_hip.check(lib.vtc_fc_dict_gradient(
      vtc_hip.ptr(X), vtc_hip.ptr(D), vtc_hip.ptr(C), vtc_hip.ptr(out), b, n,
      s, vtc_hip.ptr(ws), ws.numel(), stream), 'vtc_fc_dict_gradient')
  for _ in range(3):
    call()
  times = []
  for _ in range(reps):
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    call()
    t1.record()
    t1.synchronize()
    times.append(t0.elapsed_time(t1))
  times.sort()
  return times[len(times) // 2], times[0], times[-1]


def rel(a, ref):
  return float((a.double() - ref).norm() / ref.norm())


shapes = [(b, 256, s) for s in (1024, 256)
          for b in (1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072)]
shapes += [(131072, 64, 1024), (32768, 64, 1024), (8192, 64, 1024),
           (131072, 256, 64)]
print('%-22s %-5s %9s %9s %9s %10s  %s' % (
    '(b, n, s)', 'route', 'median ms', 'min', 'max', 'rel err', 'verdict'))
for b, n, s in shapes:
  X, D, C = problem(b, n, s)
  ws = vtc_hip.workspace(lib.vtc_fc_dict_gradient_workspace_bytes(b, n, s), dev)
  out = torch.empty(s, n, device=dev)
  ref = None
  if b <= 8192:
    ref = C.double().t() @ (C.double() @ D.double() - X.double())
  rows = {}
  for route in ROUTES:
    med, lo, hi = run(route, X, D, C, ws, out, REPS)
    rows[route] = (med, lo, hi)
    err = '%10.2e' % rel(out, ref) if ref is not None else '%10s' % '-'
    verdict = ''
    if route != 'f32':
      f = rows['f32']
      spread = max(f[2] - f[1], hi - lo)
      verdict = ('wins' if f[0] - med >= 2 * spread else
                 'loses' if med - f[0] >= 2 * spread else 'no difference')
    print('%-22s %-5s %9.4f %9.4f %9.4f %s  %s' % (
        (b, n, s), route, med, lo, hi, err, verdict))
  del X, D, C, ws, ref
