"""Times the dataset preprocessing on one device with HIP events (medians):

  1. local contrast normalisation and local luminance subtraction of a
     64-image stack at 512x512 and 1024x1536, sigma = 2, 4, 8, with the bytes
     moved (4 read + 8 written per pixel) as a fraction of the copy ceiling
     of DESIGN.md section 5 (6.4 TB/s);
  2. create_patch_training_set(131072, (16, 16), 8, stack,
     ['standardize_data_range', 'whiten_center_surround', 'patch']) on ten
     512x512 images (Field_NW's size).

and, on this machine's CPU, the reference's own operations for the same
work: scipy.signal.convolve2d(..., 'same', boundary='symm') with the float64
Gaussian window per image (filter_sd), and numpy's float64 FFT whitening per
image plus the per-patch randint loop of dataset_generation.py:205-222.

  python3 tools/time_dataset.py > profiles/dataset_timing.txt
"""
import pathlib
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent /
                       'vision-transform-codes_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from utils import dataset_generation as dg  # noqa: E402
from utils import image_processing as ip  # noqa: E402

dev = torch.device('cuda:0')
COPY_CEILING = 6.4e12


def median_ms(fn, reps):
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


def cpu_filter_s(h, w, sigma):
  """One image through the reference's filter_sd (convolve2d, float64)."""
  from scipy.signal import convolve2d
  lower, taps = ip.gaussian_window(sigma)
  v = np.arange(lower, lower + taps)
  kv, kh = np.meshgrid(v, v, indexing='ij')
  g = np.exp(-0.5 * (kv**2 + kh**2) / sigma**2)
  g /= g.sum()
  img = np.random.RandomState(0).rand(h, w).astype(np.float32)
  t = time.perf_counter()
  out = np.zeros((h, w), np.float32)
  out[:] = convolve2d(img, g, 'same', boundary='symm')
  return time.perf_counter() - t


def main():
  print('device: %s' % torch.cuda.get_device_name(dev))
  count = 64
  for h, w in ((512, 512), (1024, 1536)):
    g = torch.Generator(device=dev).manual_seed(h)
    x = torch.rand(count, h, w, 1, device=dev, generator=g) + 0.5
    px = count * h * w
    for sigma in (2, 4, 8):
      for tag, fn in (('LCN', ip.local_contrast_normalization),
                      ('LLS', ip.local_luminance_subtraction)):
        ms = median_ms(lambda: fn(x, sigma, True), 10)
        frac = 12.0 * px / (ms * 1e-3) / COPY_CEILING
        print('%s %4dx%-4d x %d  sigma %d  %8.3f ms  %6.2f us/Mpx  '
              '%5.2f TB/s = %4.0f %% of copy' % (
                  tag, h, w, count, sigma, ms, ms * 1e3 / (px / 1e6),
                  12.0 * px / (ms * 1e-3) / 1e12, 100 * frac))
        sys.stdout.flush()
      cpu = cpu_filter_s(h, w, sigma)
      print('    reference CPU filter_sd, one image: %.3f s  -> %d images '
            '%.1f s' % (cpu, count, cpu * count))
      sys.stdout.flush()
    del x
  # the examples' pipeline
  g = torch.Generator(device=dev).manual_seed(7)
  stack = torch.rand(10, 512, 512, 1, device=dev, generator=g)
  ops = ['standardize_data_range', 'whiten_center_surround', 'patch']

  def call():
    np.random.seed(0)
    return dg.create_patch_training_set(131072, (16, 16), 8, stack, ops)
  call()
  torch.cuda.synchronize()
  times = []
  for _ in range(5):
    t = time.perf_counter()
    call()
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t)
  print('create_patch_training_set(131072 x 16x16, 10 x 512x512, '
        'sdr + whiten_center_surround + patch): %.1f ms (wall, median)'
        % (1e3 * float(np.median(times))))
  # CPU: the reference's operations for the same call
  imgs = stack.cpu().numpy()
  t = time.perf_counter()
  lo, hi = imgs.min(), imgs.max()
  imgs = (imgs - lo) / (hi - lo)
  fy = np.fft.fftfreq(512)[:, None]
  fx = np.fft.fftfreq(512)[None, :]
  filt = np.sqrt(fy * fy + fx * fx) * np.exp(-(np.sqrt(fy * fy + fx * fx) /
                                               0.9)**8)
  white = [np.real(np.fft.ifft2(np.fft.fft2(imgs[i, :, :, 0]) * filt))
           .astype(np.float32)[:, :, None] for i in range(10)]
  np.random.seed(0)
  out = np.zeros((131072, 16, 16, 1), np.float32)
  for p in range(131072):
    i = np.random.randint(0, 10)
    v = np.random.randint(8, 512 - 16 - 8)
    u = np.random.randint(8, 512 - 16 - 8)
    out[p] = white[i][v:v + 16, u:u + 16]
  print('reference operations on the CPU for the same call: %.1f s'
        % (time.perf_counter() - t))


if __name__ == '__main__':
  main()
