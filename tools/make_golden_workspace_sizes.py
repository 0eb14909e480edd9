"""Records every vtc_*_workspace_bytes answer of the built library over a grid
that stands on both sides of every route switch, one call per line, into
tests/golden/workspace_sizes.txt.  The queries are host-only (no device: the
compute-unit count falls back to 256, the MI355X count), so this runs anywhere
the library builds.

Run it on the commit whose sizes are to be pinned, BEFORE touching a layout:
tests/test_workspace_sizes_host.py then holds every later commit to the file.

Line format:   <query> <arg> <arg> ... = <bytes>
  conv queries: b c h w s kh kw stride_v stride_h  (or the word `null`)
"""
import ctypes
import pathlib
import sys

REPO = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / 'vision-transform-codes_amd'))
OUT = REPO / 'tests' / 'golden' / 'workspace_sizes.txt'


def conv_args(b, c, k, stride, s, code):
  """Padded image sizes such that (code - 1) * stride + kernel == image."""
  kh, kw = k
  ch, cw = code
  return (b, c, (ch - 1) * stride + kh, (cw - 1) * stride + kw, s, kh, kw,
          stride, stride)


def grid():
  calls = []

  def add(name, *args):
    calls.append((name, args))

  # ---- fully-connected inference: small / chip16 / fused / streamed / tiled
  for n in (64, 144, 256, 100):
    for s in (64, 200, 256, 512, 576, 1024, 1280, 4096, 1000):
      for b in (1, 31, 32, 33, 250, 8192, 131072):
        for precision in range(4):
          add('vtc_fc_ista_fista_workspace_bytes', b, n, s, precision)
  for args in ((0, 256, 1024, 0), (-1, 256, 1024, 3), (32, 0, 1024, 1),
               (32, 256, 0, 2), (32, 256, -8, 0), (0, 0, 0, 0)):
    add('vtc_fc_ista_fista_workspace_bytes', *args)

  # ---- subspace inference: groups * m on both sides of 1024 (streamed route)
  for m in (1, 2, 3, 4, 8):
    below, at = 1024 // m - 1, 1024 // m
    for groups in (16, below, at, at + 1, 2 * at, 4096 // m):
      for n in (64, 256, 100):
        for b in (1, 33, 250, 8192):
          add('vtc_subspace_ista_fista_workspace_bytes', b, n, groups, m)
  for args in ((0, 256, 256, 4), (250, 0, 256, 4), (250, 256, 0, 4),
               (250, 256, 256, 0), (-250, 256, 256, 4), (250, 256, -1, 4)):
    add('vtc_subspace_ista_fista_workspace_bytes', *args)

  # ---- convolutional inference and gradient
  for k in ((5, 5), (8, 8), (11, 11), (16, 16), (8, 11)):
    for c in (1, 2, 3, 4):
      for stride in (1, 8):
        for s in (8, 32, 33, 96):
          for b in (1, 5, 8):
            for code in ((6, 9), (42, 42)):
              args = conv_args(b, c, k, stride, s, code)
              add('vtc_conv_ista_fista_workspace_bytes', *args)
              add('vtc_conv_dict_gradient_workspace_bytes', *args)
  # stride 2 and 4 (the patch contraction's cover rule), a large batch, and
  # geometries make_geo refuses
  for args in (conv_args(5, 1, (8, 8), 2, 64, (20, 20)),
               conv_args(5, 1, (16, 16), 2, 64, (20, 20)),
               conv_args(5, 3, (16, 16), 4, 64, (12, 12)),
               conv_args(128, 1, (11, 11), 1, 64, (42, 42)),
               conv_args(70000, 1, (8, 8), 1, 8, (2, 2)),
               conv_args(70000, 1, (8, 8), 8, 8, (2, 2)),
               conv_args(0, 1, (8, 8), 1, 64, (12, 12)),
               (5, 1, 50, 50, 64, 8, 8, 8, 8),      # not (code-1)*stride+k
               (5, 1, 4, 4, 64, 8, 8, 1, 1),        # kernel exceeds image
               (5, 0, 20, 20, 64, 8, 8, 1, 1),
               (5, 1, 20, 20, 0, 8, 8, 1, 1),
               (5, 1, 20, 20, 64, 8, 8, 0, 1),
               (-5, 1, 20, 20, 64, 8, 8, 1, 1)):
    add('vtc_conv_ista_fista_workspace_bytes', *args)
    add('vtc_conv_dict_gradient_workspace_bytes', *args)
  add('vtc_conv_ista_fista_workspace_bytes', 'null')
  add('vtc_conv_dict_gradient_workspace_bytes', 'null')

  # ---- dictionary updates
  for b in (1, 250, 512, 513, 8192, 131072):
    for n, s in ((64, 64), (256, 256), (256, 1024), (144, 576), (100, 1000)):
      add('vtc_fc_dict_gradient_workspace_bytes', b, n, s)
    for s in (64, 256, 1024):
      add('vtc_ica_moment_workspace_bytes', b, s)
      for positions in (1, 2, 1764):
        add('vtc_code_energy_workspace_bytes', b, s, positions)
  for args in ((0, 256, 1024), (250, 0, 1024), (250, 256, 0), (-1, 256, 1024)):
    add('vtc_fc_dict_gradient_workspace_bytes', *args)
  for args in ((0, 256), (250, 0), (-250, 256), (250, -1)):
    add('vtc_ica_moment_workspace_bytes', *args)
  for args in ((0, 256, 1), (250, 0, 1), (250, 256, 0), (250, 256, -1),
               (-1, 256, 1)):
    add('vtc_code_energy_workspace_bytes', *args)
  for slots, n in ((256, 64), (1024, 256), (1026, 100), (1, 1), (0, 256),
                   (-4, 256), (256, 0)):
    add('vtc_subspace_alignment_gradient_workspace_bytes', slots, n)
  for s, n in ((64, 64), (256, 256), (100, 144), (1024, 256), (0, 64),
               (64, 0), (-1, 64), (64, -1)):
    add('vtc_ica_apply_workspace_bytes', s, n)

  # ---- eigen-solvers, inverse, covariance, moments
  for n in (1, 2, 63, 64, 65, 100, 128, 256, 257, 512, 1024, 1025, 4096, 0,
            -1):
    add('vtc_lambda_max_workspace_bytes', n)
    add('vtc_sym_eig_workspace_bytes', n)
    add('vtc_mat_inverse_workspace_bytes', n)
  for rows in (1, 100, 4096, 100000, 1000000):
    for cols in (1, 64, 100, 256, 768, 1024):
      add('vtc_column_covariance_workspace_bytes', rows, cols)
      add('vtc_column_moments_workspace_bytes', rows, cols)
  for args in ((0, 64), (100, 0), (-1, 64), (100, -1), (100, 5000)):
    add('vtc_column_covariance_workspace_bytes', *args)
    add('vtc_column_moments_workspace_bytes', *args)

  # ---- image preprocessing
  add('vtc_window_minmax_workspace_bytes')
  for count in (1, 5, 64):
    for h, w in ((16, 16), (64, 64), (100, 120), (512, 512), (33, 47)):
      for c in (1, 3):
        add('vtc_whiten_center_surround_workspace_bytes', count, h, w, c)
        for sigma in (0.5, 2.0, 4.0, 8.0, 20.0, 50.0):
          add('vtc_local_normalize_workspace_bytes', count, h, w, c, sigma)
  for args in ((0, 64, 64, 1), (5, 0, 64, 1), (5, 64, 0, 1), (5, 64, 64, 0),
               (-5, 64, 64, 1), (5, -64, 64, 1)):
    add('vtc_whiten_center_surround_workspace_bytes', *args)
    add('vtc_local_normalize_workspace_bytes', *(args + (4.0,)))
  for sigma in (0.0, -1.0):
    add('vtc_local_normalize_workspace_bytes', 5, 64, 64, 1, sigma)
  return calls


def call(lib, name, args):
  """One query through the binding; `args` as they stand on a line."""
  import vtc_hip
  fn = getattr(lib, name)
  if 'conv' in name:
    if args == ('null',):
      return fn(None)
    b, c, h, w, s, kh, kw, sv, sh = (int(a) for a in args)
    geom = vtc_hip.ConvGeometry(b=b, c=c, h=h, w=w, s=s, kh=kh, kw=kw,
                                stride_v=sv, stride_h=sh, has_padding=0,
                                pad_lead_v=0, pad_trail_v=0, pad_lead_h=0,
                                pad_trail_h=0)
    return fn(ctypes.byref(geom))
  argtypes = vtc_hip.SIGNATURES[name][1]
  return fn(*[float(a) if t is ctypes.c_double else int(a)
              for a, t in zip(args, argtypes)])


def main():
  import vtc_hip
  lib = vtc_hip.load_library()
  lines = []
  for name, args in grid():
    text = ' '.join(repr(a) if isinstance(a, float) else str(a) for a in args)
    value = call(lib, name, tuple(str(a) for a in args))
    lines.append(('%s %s' % (name, text)).rstrip() + ' = %d\n' % value)
  OUT.write_text(''.join(lines))
  print('wrote %d lines to %s' % (len(lines), OUT))


if __name__ == '__main__':
  main()
