"""Times the three row kernels of include/vtc_codec.h -- symbol counts, stream
lengths, packing -- on 1 048 576 patches of 64 levels (256 MiB of int32),
quantised from Laplacian DCT-like codes with the Annex K.1 bin widths.
HIP-event medians of the raw C calls; bytes moved per second beside the box's
measured HBM copy rate (profiles/r03_peaks.txt).

  timeout 600 python3 tools/time_jpeg.py > profiles/jpeg_coding.txt
"""
import pathlib
import re
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import vtc_hip  # noqa: E402
from utils import jpeg  # noqa: E402

D, S = 1 << 20, 64
dev = torch.device('cuda:0')


def device_ms(fn, reps=20):
  fn()
  times = []
  for _ in range(reps):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    times.append(a.elapsed_time(b))
  return float(np.median(times))


def copy_rate():
  """TB/s of the plain HBM copy of profiles/r03_peaks.txt."""
  text = (REPO / 'profiles' / 'r03_peaks.txt').read_text()
  m = re.search(r'HBM copy\s+4 loads in flight, plain[^:]*:\s*([0-9.]+) TB/s',
                text)
  return float(m.group(1))


def main():
  lib = vtc_hip.load_library()
  stream = vtc_hip.current_stream(dev)
  p = vtc_hip.ptr
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: timeout 600 python3 tools/time_jpeg.py')
  print('%d patches x %d levels (int32, %d MiB); HIP-event medians of 20'
        % (D, S, D * S * 4 >> 20))
  widths = jpeg.get_jpeg_quant_hifi_binwidths()
  rs = np.random.RandomState(0)
  scale = 300.0 / (1.0 + np.arange(S)) ** 1.2
  levels = torch.empty((D, S), dtype=torch.int32, device=dev)
  step = 1 << 16
  for start in range(0, D, step):       # codes made and quantised in slices
    codes = (rs.laplace(size=(step, S)) * scale).astype(np.float32)
    levels[start:start + step] = jpeg.quantize(
        torch.from_numpy(codes).to(dev), widths)
  print('nonzero levels: %.1f %%' % (
      100.0 * float((levels != 0).float().mean())))

  counts = torch.empty(272, dtype=torch.int64, device=dev)
  status = torch.empty(2, dtype=torch.int32, device=dev)

  def run_counts():
    vtc_hip.check(lib.vtc_jpeg_symbol_counts(
        p(levels), D, S, p(counts), p(counts[256:]), p(status), stream),
                  'vtc_jpeg_symbol_counts')
  ms_counts = device_ms(run_counts)
  host = counts.cpu().numpy()
  tables = jpeg.tables_from_counts(host[:256], host[256:])
  t = jpeg._DeviceTables(tables[0], tables[1], dev)
  bits = torch.empty(D, dtype=torch.int32, device=dev)

  def run_bits():
    vtc_hip.check(lib.vtc_jpeg_stream_bits(
        p(levels), D, S, p(t.ac_len), p(t.dc_len), p(bits), p(status), stream),
                  'vtc_jpeg_stream_bits')
  ms_bits = device_ms(run_bits)
  assert status.tolist() == [0, 0]
  offsets = jpeg.bit_offsets(bits)
  ms_offsets = device_ms(lambda: jpeg.bit_offsets(bits))
  total = int(offsets[-1])
  out = torch.empty(-(-total // 8), dtype=torch.uint8, device=dev)

  def run_pack():
    vtc_hip.check(lib.vtc_jpeg_pack(
        p(levels), D, S, p(t.ac_code), p(t.ac_len), p(t.dc_code), p(t.dc_len),
        p(offsets), p(out), out.numel(), p(status), stream), 'vtc_jpeg_pack')
  ms_pack = device_ms(run_pack)
  assert status.tolist() == [0, 0]

  peak = copy_rate()
  level_bytes = D * S * 4
  rows = [('vtc_jpeg_symbol_counts', ms_counts, level_bytes),
          ('vtc_jpeg_stream_bits', ms_bits, level_bytes + D * 4),
          ('vtc_jpeg_bit_offsets', ms_offsets, D * 4 * 2 + (D + 1) * 8),
          ('vtc_jpeg_pack (memset included)', ms_pack,
           level_bytes + D * 8 + 2 * out.numel())]
  print('stream: %d bits = %.3f bits per level, %.1f MiB packed'
        % (total, total / float(D * S), out.numel() / 2.0 ** 20))
  for name, ms, nbytes in rows:
    rate = nbytes / (ms * 1e-3) / 1e12
    print('  %-34s %8.3f ms   %6.3f TB/s moved = %4.1f %% of the %.2f TB/s '
          'HBM copy of profiles/r03_peaks.txt'
          % (name, ms, rate, 100.0 * rate / peak, peak))
  print('reference (utils/jpeg.py, pure Python), measured on a DIFFERENT '
        'machine (a CPU host) at 20 000 patches of 64:')
  print('  generate_ac_dc_huffman_tables 0.73 s (about 36 s scaled to 10^6 '
        'patches); streams 47 us per patch, 0.94 s (about 47 s scaled)')


if __name__ == '__main__':
  main()
