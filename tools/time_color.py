"""Times the three kernels of include/ext/vtc_color.h on one device: a stack
of 24 x 512 x 768 x 3 float32, the size of the Kodak set, and once 131 072
patches of 8 x 8 x 3.  The raw entry points on preallocated arrays, HIP-event
medians of windows of 20 calls; bytes per second are the bytes the call must
read and write over that time, beside a device copy of as many bytes timed in
the same run.

  python3 tools/time_color.py > profiles/color.txt
"""
import ctypes
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent /
                       'vision-transform-codes_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vtc_hip  # noqa: E402
from utils import color  # noqa: E402

dev = torch.device('cuda:0')
CALLS, WINDOWS = 20, 15


def window_ms(fn):
  """Median over WINDOWS of the time of CALLS back-to-back calls, per call."""
  for _ in range(3):
    fn()
  torch.cuda.synchronize(dev)
  times = []
  for _ in range(WINDOWS):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
      fn()
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b) / CALLS)
  return float(np.median(times)), float(np.min(times)), float(np.max(times))


def doubles(values):
  values = np.asarray(values, dtype=np.float64).reshape(-1).tolist()
  return (ctypes.c_double * len(values))(*values)


def report(name, nbytes, fn):
  ms, lo, hi = window_ms(fn)
  print('  %-44s %8.4f ms (%.4f .. %.4f)  %7.1f MB  %6.2f TB/s' % (
      name, ms, lo, hi, nbytes / 1e6, nbytes / ms / 1e9))
  sys.stdout.flush()


def copy_rate(nbytes):
  """A device copy that reads nbytes / 2 and writes nbytes / 2."""
  src = torch.empty(nbytes // 8, dtype=torch.float32, device=dev).normal_()
  dst = torch.empty_like(src)
  report('device copy of as many bytes', 2 * src.numel() * 4,
         lambda: dst.copy_(src))


def transforms(lib, stream, count, h, w):
  forward = doubles(color.JFIF_FORWARD)
  inverse = doubles(color.JFIF_INVERSE)
  zero, offset = doubles([0., 0., 0.]), doubles([0., 128., 128.])
  void = lambda v: ctypes.cast(v, ctypes.c_void_p)
  x = torch.rand(count, h, w, 3, device=dev) * 255.
  arena = torch.empty(x.numel() + 4, dtype=torch.float32, device=dev)
  skewed = arena[1:1 + x.numel()]
  skewed.copy_(x.reshape(-1))
  out = torch.empty(x.numel() + 4, dtype=torch.float32, device=dev)
  nbytes = 2 * 4 * x.numel()
  rows = [('forward JFIF hwc -> hwc', x, 0, out, 0, forward, zero, offset, 0),
          ('forward JFIF hwc -> chw', x, 0, out, 1, forward, zero, offset, 0),
          ('inverse JFIF chw -> hwc, clamped', x, 1, out, 0, inverse, offset,
           zero, 1),
          ('inverse JFIF chw -> chw', x, 1, out, 1, inverse, offset, zero, 0),
          ('forward JFIF hwc -> chw, +4 bytes (by element)', skewed, 0,
           out[1:], 1, forward, zero, offset, 0)]
  for name, src, a, dst, b, m, pre, post, clamp in rows:
    def call():
      vtc_hip.check(lib.vtc_color_transform(
          vtc_hip.ptr(src), a, vtc_hip.ptr(dst), b, count, h, w, void(m),
          void(pre), void(post), clamp, 0., 255., stream),
                    'vtc_color_transform')
    report(name, nbytes, call)
  copy_rate(nbytes)


def resamplers(lib, stream, count, h, w):
  x = torch.rand(count, h, w, device=dev) * 255.
  for fv, fh in ((2, 2), (1, 2), (4, 4)):
    hs, ws = -(-h // fv), -(-w // fh)
    small = torch.empty(count, hs, ws, dtype=torch.float32, device=dev)
    back = torch.empty(count, h, w, dtype=torch.float32, device=dev)
    nbytes = 4 * (x.numel() + small.numel())

    def down():
      vtc_hip.check(lib.vtc_plane_downsample(
          vtc_hip.ptr(x), vtc_hip.ptr(small), count, h, w, fv, fh, stream),
                    'vtc_plane_downsample')
    report('downsample %d x %d' % (fv, fh), nbytes, down)
    for mode, name in ((vtc_hip.UPSAMPLE_REPLICATE, 'replicate'),
                       (vtc_hip.UPSAMPLE_TRIANGLE, 'triangle')):
      def up():
        vtc_hip.check(lib.vtc_plane_upsample(
            vtc_hip.ptr(small), vtc_hip.ptr(back), count, hs, ws, h, w, fv,
            fh, mode, stream), 'vtc_plane_upsample')
      report('upsample %d x %d %s' % (fv, fh, name), nbytes, up)
  copy_rate(4 * (x.numel() + x.numel() // 4))


def main():
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: python3 tools/time_color.py')
  print('HIP-event medians (min .. max) of %d windows of %d calls; bytes: '
        'what the call must read plus what it must write' % (WINDOWS, CALLS))
  for count, h, w, what in ((24, 512, 768, 'the Kodak set'),
                            (131072, 8, 8, '131 072 patches of 8 x 8 x 3')):
    print('%d x %d x %d x 3 (%s)' % (count, h, w, what))
    transforms(lib, stream, count, h, w)
    if count == 24:
      print('2 x %d x %d x %d planes (Cb and Cr of it)' % (count, h, w))
      resamplers(lib, stream, 2 * count, h, w)


if __name__ == '__main__':
  main()
