"""Times the baseline JFIF writer of include/ext/vtc_jfif.h on one device: a
seeded 768 x 512 colour image at 4:2:0, quality 75 and quality 95.  Each raw C
call of the chain on preallocated arrays (HIP-event medians of windows of 20
calls, after warm-up), utils.jfif.encode_rgb end to end (host table building
and its reads included, wall clock around a synchronise), the size of the
file, and PIL's own encoder on the host of the same box for scale.

  python3 tools/time_jfif.py > profiles/jfif.txt
"""
import io
import pathlib
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent /
                       'vision-transform-codes_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vtc_hip  # noqa: E402
from utils import color, jfif  # noqa: E402

dev = torch.device('cuda:0')
CALLS, WINDOWS = 20, 15
H, W = 512, 768


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


def report(name, fn):
  ms, lo, hi = window_ms(fn)
  print('  %-46s %8.4f ms (%.4f .. %.4f)' % (name, ms, lo, hi))
  sys.stdout.flush()
  return ms


def picture():
  """(H, W, 3) float32 in [0, 255]: smooth colour fields, edges and noise."""
  rs = np.random.RandomState(768512)
  y, x = np.mgrid[0:H, 0:W].astype(np.float64)
  planes = []
  for c in range(3):
    p = (128. + 60. * np.sin(x / (23. + 7 * c)) * np.cos(y / (31. - 5 * c)) +
         40. * ((x // 64 + y // 48 + c) % 2) + 25. * np.sin((x + y) / 3.1) +
         8. * rs.randn(H, W))
    planes.append(p)
  return np.clip(np.stack(planes, axis=-1), 0., 255.).astype(np.float32)


def chain(lib, stream, image, quality):
  up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
  layout = jfif.scan_layout((H, W), (2, 2))
  planes = color.split_planes(image, (2, 2))
  luma, chroma = jfif.quality_tables(quality)
  d = layout['rows']
  levels = torch.empty((d, 64), dtype=torch.int32, device=dev)
  basis = up(jfif.dct_basis())
  total = 0.
  for c, plane in enumerate(planes):
    q = up((luma if c == 0 else chroma).view(np.int16))
    rob = up(layout['row_of_block'][c])
    h, w = plane.shape
    bh, bw = layout['grids'][c]

    def forward():
      vtc_hip.check(lib.vtc_jfif_forward_dct(
          vtc_hip.ptr(plane), h, w, bh, bw, vtc_hip.ptr(basis),
          vtc_hip.ptr(q), vtc_hip.ptr(rob), vtc_hip.ptr(levels), d, stream),
                    'vtc_jfif_forward_dct')
    total += report('vtc_jfif_forward_dct %s %d x %d' % ('Y Cb Cr'.split()[c],
                                                         h, w), forward)
  pred, sel = up(layout['pred']), up(layout['table_sel'])
  counts = torch.empty(2 * 256 + 2 * 16, dtype=torch.int64, device=dev)
  status = torch.empty(2, dtype=torch.int32, device=dev)

  def count():
    vtc_hip.check(lib.vtc_jfif_symbol_counts(
        vtc_hip.ptr(levels), d, vtc_hip.ptr(pred), vtc_hip.ptr(sel),
        vtc_hip.ptr(counts), vtc_hip.ptr(counts[512:]), vtc_hip.ptr(status),
        stream), 'vtc_jfif_symbol_counts')
  total += report('vtc_jfif_symbol_counts, %d blocks' % d, count)
  host = counts.cpu().numpy()
  ac, dc = host[:512].reshape(2, 256), host[512:].reshape(2, 16)
  t0 = time.perf_counter()
  tables = jfif.tables_from_counts(ac, dc)
  tables_ms = (time.perf_counter() - t0) * 1e3
  tab = jfif._DeviceTables(tables, dev)
  bits = torch.empty(d, dtype=torch.int32, device=dev)

  def block_bits():
    vtc_hip.check(lib.vtc_jfif_block_bits(
        vtc_hip.ptr(levels), d, vtc_hip.ptr(pred), vtc_hip.ptr(sel),
        vtc_hip.ptr(tab.ac_len), vtc_hip.ptr(tab.dc_len), vtc_hip.ptr(bits),
        vtc_hip.ptr(status), stream), 'vtc_jfif_block_bits')
  total += report('vtc_jfif_block_bits', block_bits)
  offsets = torch.empty(d + 1, dtype=torch.int64, device=dev)
  ws = vtc_hip.workspace(lib.vtc_jpeg_bit_offsets_workspace_bytes(d), dev)

  def scan():
    vtc_hip.check(lib.vtc_jpeg_bit_offsets(
        vtc_hip.ptr(bits), d, vtc_hip.ptr(offsets), vtc_hip.ptr(ws),
        ws.numel(), stream), 'vtc_jpeg_bit_offsets')
  total += report('vtc_jpeg_bit_offsets', scan)
  nbytes = -(-int(offsets[d]) // 8)
  raw = torch.empty(nbytes, dtype=torch.uint8, device=dev)

  def pack():
    vtc_hip.check(lib.vtc_jfif_pack(
        vtc_hip.ptr(levels), d, vtc_hip.ptr(pred), vtc_hip.ptr(sel),
        vtc_hip.ptr(tab.ac_code), vtc_hip.ptr(tab.ac_len),
        vtc_hip.ptr(tab.dc_code), vtc_hip.ptr(tab.dc_len),
        vtc_hip.ptr(offsets), vtc_hip.ptr(raw), nbytes, vtc_hip.ptr(status),
        stream), 'vtc_jfif_pack')
  total += report('vtc_jfif_pack, %d bytes' % nbytes, pack)
  out = torch.empty(2 * nbytes, dtype=torch.uint8, device=dev)
  length = torch.empty(1, dtype=torch.int64, device=dev)
  ws2 = vtc_hip.workspace(lib.vtc_jfif_stuff_bytes_workspace_bytes(nbytes),
                          dev)

  def stuff():
    vtc_hip.check(lib.vtc_jfif_stuff_bytes(
        vtc_hip.ptr(raw), nbytes, vtc_hip.ptr(out), out.numel(),
        vtc_hip.ptr(length), vtc_hip.ptr(status), vtc_hip.ptr(ws2),
        ws2.numel(), stream), 'vtc_jfif_stuff_bytes')
  stuff()
  total += report('vtc_jfif_stuff_bytes, %d zeros inserted'
                  % (int(length[0]) - nbytes), stuff)
  print('  %-46s %8.4f ms' % ('sum of the device calls', total))
  print('  %-46s %8.4f ms' % ('host: tables_from_counts (package-merge)',
                              tables_ms))


def end_to_end(image, quality):
  times = []
  for i in range(8):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    data, info = jfif.encode_rgb(image, (2, 2), quality)
    torch.cuda.synchronize(dev)
    times.append((time.perf_counter() - t0) * 1e3)
  print('  %-46s %8.3f ms (median of the last 5 of 8, wall clock)'
        % ('utils.jfif.encode_rgb end to end', np.median(times[3:])))
  print('  file: %d bytes (%d of them headers and tables), %.3f bits per '
        'pixel, %d zeros stuffed' % (len(data), info['header_bytes'],
                                     info['bits_per_pixel'],
                                     info['stuffed_bytes']))
  return data


def pil_encoder(host, quality, ours):
  try:
    from PIL import Image
  except ImportError:
    print('  PIL is not installed: no host encoder for scale')
    return
  picture8 = Image.fromarray(np.rint(host).astype(np.uint8))
  times = []
  for _ in range(8):
    buf = io.BytesIO()
    t0 = time.perf_counter()
    picture8.save(buf, format='JPEG', quality=quality, optimize=True,
                  subsampling='4:2:0')
    times.append((time.perf_counter() - t0) * 1e3)
  print('  %-46s %8.3f ms (median of the last 5 of 8, wall clock, one host '
        'thread), %d bytes' % ('PIL save(optimize=True, 4:2:0) on the host',
                               np.median(times[3:]), len(buf.getvalue())))
  opened = Image.open(io.BytesIO(ours))
  opened.load()
  print('  PIL opens the device file: %s %s' % (opened.mode, opened.size))


def main():
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  host = picture()
  image = torch.from_numpy(host).to(dev)
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: python3 tools/time_jfif.py')
  print('%d x %d x 3 float32 image, YCbCr 4:2:0; HIP-event medians (min .. '
        'max) of %d windows of %d raw C calls after 3 warm-up calls'
        % (W, H, WINDOWS, CALLS))
  for quality in (75, 95):
    print('quality %d' % quality)
    chain(lib, stream, image, quality)
    data = end_to_end(image, quality)
    pil_encoder(host, quality, data)


if __name__ == '__main__':
  main()
