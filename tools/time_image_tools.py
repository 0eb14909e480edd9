"""Times the image-level functions of utils.image_processing on one device
(HIP-event medians) next to numpy / scipy on the host (wall-clock medians,
with torch.cuda.synchronize around them), at 512 x 512 x 1 and 512 x 768 x 3.

  python3 tools/time_image_tools.py > profiles/image_tools.txt
"""
import pathlib
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent /
                       'vision-transform-codes_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.ndimage import convolve1d  # noqa: E402
from scipy.signal import convolve2d  # noqa: E402

from utils import image_processing as ip  # noqa: E402

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


def host_ms(fn, reps=3):
  times = []
  for _ in range(reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    times.append(1e3 * (time.perf_counter() - t0))
  return float(np.median(times))


def host_filter_fd(img, filt):
  out = np.zeros(img.shape, dtype=np.float32)
  for ch in range(img.shape[2]):
    out[:, :, ch] = np.real(np.fft.ifft2(
        filt * np.fft.fft2(img[:, :, ch], filt.shape),
        filt.shape)).astype(np.float32)[:img.shape[0], :img.shape[1]]
  return out


def host_filter_sd(img, filt):
  return np.stack([convolve2d(img[:, :, ch], filt, 'same', boundary='symm')
                   for ch in range(img.shape[2])], axis=2).astype(np.float32)


def host_separable(img, vert, horz):
  mid = convolve1d(img, horz, axis=1, mode='reflect')
  return convolve1d(mid, vert, axis=0, mode='reflect')


def host_tile(img, ph, pw):
  ny, nx = img.shape[0] // ph, img.shape[1] // pw
  return np.ascontiguousarray(
      img[:ny * ph, :nx * pw].reshape(ny, ph, nx, pw, -1).transpose(
          0, 2, 1, 3, 4)).reshape(ny * nx, ph, pw, -1)


def host_assemble(patches, ph, pw, positions, shape):
  out = np.zeros(shape, dtype=patches.dtype)
  for p, (v, u) in enumerate(positions):
    out[v:v + ph, u:u + pw] = patches[p]
  return out


def main():
  print('device: %s' % torch.cuda.get_device_name(dev))
  print('command: python3 tools/time_image_tools.py')
  print('device: HIP-event medians of 20; host: numpy / scipy wall-clock '
        'medians of 3')
  rs = np.random.RandomState(0)
  for h, w, c in ((512, 512, 1), (512, 768, 3)):
    img = rs.rand(h, w, c).astype(np.float32)
    dimg = torch.from_numpy(img).to(dev)
    lpf = ip.get_low_pass_filter((h, w), {'shape': 'exponential',
                                          'cutoff': 0.3, 'order': 4.0})
    dlpf = torch.from_numpy(lpf).to(dev)
    f7 = rs.randn(7, 7)
    f31 = rs.randn(31, 31)
    d7, d31 = torch.from_numpy(f7).to(dev), torch.from_numpy(f31).to(dev)
    vert, horz = ip.get_binomial_filter_1d(9), ip.get_binomial_filter_1d(9)
    dvert, dhorz = torch.from_numpy(vert).to(dev), torch.from_numpy(horz).to(dev)
    patches, positions = ip.patches_from_single_image(dimg, (16, 16), False)
    hpatches = patches.cpu().numpy()
    rows = [
        ('filter_fd', lambda: ip.filter_fd(dimg, dlpf),
         lambda: host_filter_fd(img, lpf)),
        ('filter_sd 7x7', lambda: ip.filter_sd(dimg, d7),
         lambda: host_filter_sd(img, f7)),
        ('filter_sd 31x31', lambda: ip.filter_sd(dimg, d31),
         lambda: host_filter_sd(img, f31)),
        ('filter_sd separable 9+9',
         lambda: ip.filter_sd(dimg, None, dvert, dhorz),
         lambda: host_separable(img, vert, horz)),
        ('downsample 2', lambda: ip.downsample(dimg, 2),
         lambda: np.ascontiguousarray(img[::2, ::2])),
        ('patches_from_single_image 16x16',
         lambda: ip.patches_from_single_image(dimg, (16, 16), False),
         lambda: host_tile(img, 16, 16)),
        ('assemble_image_from_patches',
         lambda: ip.assemble_image_from_patches(patches, (16, 16), positions),
         lambda: host_assemble(hpatches, 16, 16, positions, img.shape)),
        ('unwhiten_center_surround (ramp)',
         lambda: ip.unwhiten_center_surround(dimg, low_cutoff=0.05),
         lambda: host_filter_fd(img, 1. / np.maximum(
             ip.get_whitening_ramp_filter((h, w), False).real, 0.05))),
    ]
    print('%d x %d x %d' % (h, w, c))
    for name, on_device, on_host in rows:
      print('  %-34s device %9.3f ms   host %10.3f ms' % (
          name, device_ms(on_device), host_ms(on_host)))
      sys.stdout.flush()


if __name__ == '__main__':
  main()
