"""Cases, dispatch mirror and float64 references behind
tests/test_conv_routes_gpu.py and tests/test_conv_gates_host.py.

vtc_conv_ista_fista (csrc/conv.hip) picks one of five kernel families from the
geometry, the precision, an LDS budget and the CU count, and cx_fill_plan
(csrc/conv_x3.h) makes further choices inside the split routes.  conv_route
restates that choice; every case below names the tuple it must give.  Nothing
here needs a GPU."""
import collections
import functools

import numpy as np
import torch

import helpers
import sc_oracle

ceil_div = lambda a, b: -(-a // b)

T = 12                  # FISTA iterations of every plain case
WARM_FROM, WARM_ITERS = 5, 7
STOP_ITERS = 100
STOP_MARGIN = 0.02      # the mean step misses stop_eps by 2 % on either side
ACTIVE_BAND = (0.1, 0.9)
MAX_CODE = 10.0         # the iterates did not grow
HARD_CUTOFF = 1e-3      # lambda * eta of the hard-threshold run
HARD_ETA = 0.02         # its step (tests/test_conv_gpu.py), see hard_step
HARD_GATE = (2e-3, 1.1e-3)   # tests/test_conv_gpu.py, one iteration

GATE_F32 = (helpers.REL_TOL_SHORT, helpers.NEAR_THRESHOLD)
GATE_BF16 = (2e-5, 1e-5)     # tests/test_conv_gpu.py


# ------------------------------------------------------------ dispatch mirror
Geom = collections.namedtuple(
    'Geom', 'b c h w s kh kw stride_v stride_h has_padding pad_lead_v '
    'pad_trail_v pad_lead_h pad_trail_h')

UNIT_TY, UNIT_TX, UNIT_SYN_CHUNK = 32, 64, 4        # csrc/conv_unit.h
X3_KERNELS = (5, 8, 11, 16)
X3_STRIP, X3_ANA_MAX_ROWS, X3_ANA_PITCH = 64, 8, 88  # csrc/conv_x3.h


def code_dims(g):
  """code_dim (csrc/conv.hip) of a geometry make_geo accepts."""
  assert (g.h - g.kh) % g.stride_v == 0 and (g.w - g.kw) % g.stride_h == 0
  return (g.h - g.kh) // g.stride_v + 1, (g.w - g.kw) // g.stride_h + 1


def cover(g):
  """Code positions over one pixel."""
  return ceil_div(g.kh, g.stride_v) * ceil_div(g.kw, g.stride_h)


def patch_geometry(g):
  """patch_geometry (csrc/conv_patch.h)."""
  ch, cw = code_dims(g)
  return ((g.stride_v > 1 or g.stride_h > 1) and cover(g) <= 16 and
          g.c * g.kh * g.kw <= 8192 and g.b <= 65535 and
          g.b * ch * cw < (1 << 31))


def unit_geometry(g):
  """unit_geometry (csrc/conv_unit.h)."""
  return (g.stride_v == 1 and g.stride_h == 1 and g.kh == g.kw and
          g.kh in X3_KERNELS)


def unit_analysis_bytes(g):
  wy, wx = UNIT_TY + g.kh - 1, (UNIT_TX + g.kw - 1 + 3) // 4 * 4
  kp = (g.kw + 3) // 4 * 4
  return (g.c * wy * wx + g.s * g.c * g.kh * kp) * 4


def unit_analysis_fits(g):
  """unit_analysis_fits (csrc/conv_unit.h): window of all channels and the
  taps of all kernels within 140 KiB."""
  return unit_analysis_bytes(g) <= 140 * 1024


def unit_groups(g, tiles):
  """unit_groups (csrc/conv_unit.h): (blocks that share a tile's kernels,
  kernels per block)."""
  want = ceil_div(1536, tiles * g.b)
  want = max(min(want, ceil_div(g.s, 4 * UNIT_SYN_CHUNK), 8), 1)
  per = ceil_div(ceil_div(g.s, want), UNIT_SYN_CHUNK) * UNIT_SYN_CHUNK
  return ceil_div(g.s, per), per


def plan_analysis(g):
  """plan_analysis (csrc/conv.hip): (tp, tq, window bytes), the tile halved
  until the residual window of all channels fits 40 KiB."""
  tp = tq = 16
  while True:
    wy, wx = (tp - 1) * g.stride_v + g.kh, (tq - 1) * g.stride_h + g.kw
    lds = g.c * wy * wx * 4
    if lds <= 40 * 1024 or (tp == 1 and tq == 1):
      return tp, tq, lds
    if tp >= tq and tp > 1:
      tp //= 2
    else:
      tq //= 2


def x3_slots(k):
  """CxDims<K>::SLOTS."""
  return 32 * ceil_div((k + 1) // 2 * k, 16)


def x3_fused_lds(k):
  """CxFused<K>::lds."""
  th = 8 + k - 1
  ana = 2 * k * 64 * 16 * 2
  syn = 2 * x3_slots(k) * (64 + 8) * 2
  win = 2 * (4 * (2 * th * 48 + 32)) * 2
  priv = 2 * 8 * k * 48 * 4
  return ana + syn + win + priv


X3Plan = collections.namedtuple(
    'X3Plan', 'AC chunks syn_chunks ana_shift ana_rows ana_lds blocks8 fused '
    'supported')


def x3_plan(g, cus):
  """The fields of cx_fill_plan / cx_plan (csrc/conv_x3.h) that change the
  code that runs.  cx_pick_rows, a cost model, is not restated: `supported`
  holds the other conditions of cx_plan, and the GPU tests compare it with
  vtc_conv_x3_supported.  None where the geometry has no split form."""
  if not (1 <= g.c <= 8 and unit_geometry(g)):
    return None
  k = g.kh
  ch, cw = code_dims(g)
  slots = x3_slots(k)
  all16 = ceil_div(g.s, 16) * 16
  parts, per = 1, all16
  while 2 * slots * (per + 8) * 2 > 100 * 1024 and per > 16:
    parts += 1
    per = ceil_div(all16 // 16, parts) * 16
  syn_chunks = ceil_div(all16, per)
  AC = 64 if g.s > 32 and g.c * 2 * k * 64 * 16 * 2 <= 100 * 1024 else 32
  chunks = ceil_div(g.s, AC)
  blocks8 = (ceil_div(cw, X3_STRIP) * ceil_div(ch, X3_ANA_MAX_ROWS) * chunks *
             g.b)
  ana_rows = 4 if blocks8 < 16 * cus else 8
  planes = 2 * k * AC * 16 * 2
  win = (ana_rows + k - 1) * X3_ANA_PITCH
  plain = g.c * (planes + 2 * win * 2)
  shifted = g.c * (planes + 4 * (2 * win + 32) * 2)
  two = g.c * (planes + 2 * (2 * win + 32) * 2)
  budget, lds = 150 * 1024, 160 * 1024
  blocks_plain = min(lds // plain, 2)
  ana_shift, ana_lds = 1, plain
  if shifted <= budget and lds // shifted >= blocks_plain:
    ana_shift, ana_lds = 4, shifted
  elif two <= budget and lds // two >= blocks_plain:
    ana_shift, ana_lds = 2, two
  fused = (g.c == 1 and AC == 64 and k <= 11 and
           x3_fused_lds(k) <= 160 * 1024)
  if fused:
    items = g.b * ceil_div(ch, 8) * ceil_div(cw, 32) * chunks
    tile_stride = ceil_div((8 + k - 1) * (32 + k - 1), 32) * 32
    if items * 8 * 2 * 1024 * 4 >= 1 << 32 or items * tile_stride * 4 >= 1 << 32:
      fused = False
  supported = (ana_lds <= budget and g.b <= 65535 and
               per * syn_chunks * ch * cw * 4 < 0x7fffffff)
  return X3Plan(AC, chunks, syn_chunks, ana_shift, ana_rows, ana_lds, blocks8,
                fused, supported)


def resolve_precision(precision, g, hard_threshold, supported):
  """_resolve_precision of analysis_transforms/convolutional/ista_fista.py:
  'auto' is the f16 split for 32 kernels or more, a soft threshold and a
  geometry vtc_conv_x3_supported accepts, else exact f32."""
  if precision != 'auto':
    return precision
  return 'f16x3' if g.s >= 32 and not hard_threshold and supported else 'f32'


def conv_route(g, precision, cus):
  """The route of vtc_conv_ista_fista.  f32: (family, syn_groups, ana_groups,
  (tp, tq)) with family in patch | unit | unit-synth+direct | direct, group
  counts 1 off the unit route, (tp, tq) of plan_analysis where the direct
  analysis runs and None elsewhere.  Split modes: ('x3-fused' | 'x3-two',
  split, AC, chunks, ragged, syn_chunks, ana_shift, ana_rows); ragged: the
  last atom chunk is partial."""
  if precision in ('f16x3', 'bf16x3'):
    p = x3_plan(g, cus)
    assert p is not None and p.supported, 'no split route for this geometry'
    return ('x3-fused' if p.fused else 'x3-two', precision[:-2], p.AC,
            p.chunks, g.s % p.AC != 0, p.syn_chunks, p.ana_shift, p.ana_rows)
  assert precision == 'f32', precision
  if patch_geometry(g):
    return ('patch', 1, 1, None)
  tiles = plan_analysis(g)[:2]
  if not unit_geometry(g):
    return ('direct', 1, 1, tiles)
  if not unit_analysis_fits(g):
    return ('unit-synth+direct', 1, 1, tiles)
  ch, cw = code_dims(g)
  syn = unit_groups(g, ceil_div(g.w, UNIT_TX) * ceil_div(g.h, UNIT_TY))[0]
  ana = unit_groups(g, ceil_div(cw, UNIT_TX) * ceil_div(ch, UNIT_TY))[0]
  return ('unit', syn, ana, None)


def family(route):
  return 'unit' if route[0] == 'unit-synth+direct' else route[0]


def gate(route):
  """(relative l2 error, largest tolerated support flip) of a route."""
  return GATE_BF16 if route[1] == 'bf16' else GATE_F32


# ---------------------------------------------------------------------- cases
# image: the un-padded (height, width); with pad None the size of the images
# as they are.  pad: 'ref' (sc_oracle.conv_padding_amount), None, or
# ((lead_v, trail_v), (lead_h, trail_h)).  sample: how many images meet the
# oracle (None: all).  stop_eps: early-stopping epsilon of the options test,
# None where the case has no options.
Case = collections.namedtuple(
    'Case', 'name precision kernel stride s c b image pad lam route stop_eps '
    'sample')

REF = 'ref'


def _cases():
  out = []

  def add(name, precision, k, stride, s, c, b, image, pad, lam, route,
          stop_eps=None, sample=None):
    kernel = k if isinstance(k, tuple) else (k, k)
    if precision == 'both':
      for prec in ('f16x3', 'bf16x3'):
        out.append(Case('%s %s' % (name, prec), prec, kernel, stride, s, c, b,
                        image, pad, lam, (route[0], prec[:-2]) + route[1:],
                        stop_eps, sample))
    else:
      out.append(Case(name, precision, kernel, stride, s, c, b, image, pad,
                      lam, route, stop_eps, sample))

  one = (1, 1)
  # route tuples of the split modes after (family, split):
  # AC, chunks, ragged, syn_chunks, ana_shift, ana_rows
  add('1 fused chunks=1', 'both', 5, one, 64, 1, 2, (29, 45), REF, LAM[1],
      ('x3-fused', 64, 1, False, 1, 4, 4))
  add('2 fused ragged chunk', 'both', 11, one, 72, 1, 2, (23, 41), REF,
      LAM[2], ('x3-fused', 64, 2, True, 1, 4, 4), STOP[2])
  # 640 bytes per atom of 11x11 synthesis planes: 100 KB hold 9 x 16 atoms
  add('3 fused syn_chunks=2', 'both', 11, one, 208, 1, 1, (24, 24), REF,
      LAM[3], ('x3-fused', 64, 4, True, 2, 4, 4))
  # 26 x 41 code map: 3 1/4 bands of 8 rows, 1 9/32 items of 32 columns;
  # asymmetric frame
  add('4 fused k=8 ragged items', 'both', 8, one, 40, 1, 3, (19, 37),
      ((5, 9), (7, 4)), LAM[4], ('x3-fused', 64, 1, True, 1, 4, 4))
  # 1024 bytes per atom of 16x16 synthesis planes: 100 KB hold 5 x 16 atoms;
  # four window copies beside the 64-atom planes would cost the second
  # resident block: two (ana_shift = 2 at AC = 64)
  add('5 two k=16 syn_chunks=2', 'both', 16, one, 100, 1, 2, (30, 44), REF,
      LAM[5], ('x3-two', 64, 2, True, 2, 2, 4), STOP[5])
  add('6 two s<=32 AC=32', 'f16x3', 11, one, 20, 1, 2, (30, 30), REF, LAM[6],
      ('x3-two', 'f16', 32, 1, True, 1, 4, 4))
  # 3 channels of 11x11 planes pass 100 KB at 64 atoms; asymmetric frame
  add('7 two c=3 AC=32 ragged', 'both', 11, one, 40, 3, 2, (21, 27),
      ((10, 6), (4, 9)), LAM[7], ('x3-two', 32, 2, True, 1, 4, 4), STOP[7])
  add('8 two c=3 k=16 ana_shift=2', 'bf16x3', 16, one, 20, 3, 2, (18, 22),
      REF, LAM['8 c=3'], ('x3-two', 'bf16', 32, 1, True, 1, 2, 4))
  add('8 two c=8 k=5 ana_shift=2', 'f16x3', 5, one, 24, 8, 2, (17, 21), REF,
      LAM['8 c=8'], ('x3-two', 'f16', 32, 1, True, 1, 2, 4))
  # 7 channels of 8x8: neither two nor four window copies fit beside the
  # kernel planes (169 792 and 224 896 bytes against 150 KiB)
  add('9 two c=7 k=8 ana_shift=1', 'f16x3', 8, one, 24, 7, 1, (17, 21), REF,
      LAM[9], ('x3-two', 'f16', 32, 1, True, 1, 1, 4))
  # 2 bands of 8 rows x 2048 images = 4096 = 16 * 256 blocks8
  add('10 two ana_rows=8', 'f16x3', 5, one, 32, 1, 2048, (12, 4), REF,
      LAM[10], ('x3-two', 'f16', 32, 1, False, 1, 4, 8), sample=8)
  # one 32 x 64 tile; 40 kernels in groups of 16, 16 and 8; asymmetric frame
  add('11 unit 3 groups', 'f32', 8, one, 40, 1, 1, (17, 46), ((7, 5), (4, 6)),
      LAM[11], ('unit', 3, 3, None), STOP[11])
  # 36 x 36 padded: 2 image tiles -> 2 groups, one 32 x 32 code tile -> 4
  add('12 unit groups differ', 'f32', 5, one, 64, 1, 384, (28, 28), REF,
      LAM[12], ('unit', 2, 4, None), sample=4)
  add('13 unit c=3 ragged tiles', 'f32', 11, one, 9, 3, 2, (25, 50), REF,
      LAM[13], ('unit', 1, 1, None))
  # (47 * 80 + 128 * 16 * 16) * 4 = 146 112 bytes against 143 360
  add('14 unit synthesis, direct analysis', 'f32', 16, one, 128, 1, 1,
      (20, 24), REF, LAM[14], ('unit-synth+direct', 1, 1, (16, 16)), STOP[14])
  # cover 6 * 5 = 30; 23 x 20 code map: two ragged tiles either way; an
  # asymmetric frame whose padded size is (code - 1) * stride + kernel
  add('15 direct strided non-square', 'f32', (11, 13), (2, 3), 13, 2, 2,
      (37, 50), ((7, 11), (11, 9)), LAM[15], ('direct', 1, 1, (16, 16)),
      STOP[15])
  # 8 * 43 * 43 * 4 = 59 168 bytes > 40 KiB -> 8 x 16 tile (37 152).  No
  # reference frame exists for an odd kernel at stride 2 (the padded size is
  # never (code - 1) * 2 + 13): lead 11, trail 12
  add('16 direct shrunk tile', 'f32', 13, (2, 2), 6, 8, 2, (24, 30),
      ((11, 12), (11, 12)), LAM[16], ('direct', 1, 1, (8, 16)))
  add('17 direct stride 1 k=7 no padding', 'f32', 7, one, 34, 3, 2, (29, 40),
      None, LAM[17], ('direct', 1, 1, (16, 16)))
  add('18 patch non-square', 'f32', (4, 6), (2, 3), 7, 3, 3, (21, 20),
      ((2, 3), (3, 4)), LAM[18], ('patch', 1, 1, None), STOP[18])
  add('19 patch k=16 stride 8', 'f32', 16, (8, 8), 24, 1, 5, (40, 56), REF,
      LAM[19], ('patch', 1, 1, None))
  # a trailing pad of 0 blanks the axis (the `-0:` slice of the reference's
  # mask) and with it the whole residual: the codes stay exactly zero
  add('20 fused blank rows', 'f16x3', 5, one, 64, 1, 2, (33, 45),
      ((4, 0), (4, 4)), 0.3, ('x3-fused', 'f16', 64, 1, False, 1, 4, 4))
  add('21 two blank columns', 'bf16x3', 11, one, 20, 1, 2, (30, 40),
      ((10, 10), (10, 0)), 0.3, ('x3-two', 'bf16', 32, 1, True, 1, 4, 4))
  add('22 unit blank columns', 'f32', 8, one, 40, 1, 1, (17, 52),
      ((7, 5), (4, 0)), 0.3, ('unit', 3, 3, None))
  add('23 direct blank rows', 'f32', (11, 13), (2, 3), 13, 2, 2, (48, 50),
      ((7, 0), (11, 9)), 0.3, ('direct', 1, 1, (16, 16)))
  add('24 patch blank rows', 'f32', (4, 6), (2, 3), 7, 3, 3, (24, 20),
      ((2, 0), (3, 4)), 0.3, ('patch', 1, 1, None))
  return out


# sparsity weights and early-stopping epsilons, found on the CPU (see
# assert_input_conditions and stop_reference; tests/test_conv_gates_host.py
# checks every one)
LAM = {1: 0.05, 2: 0.1, 3: 0.05, 4: 0.1, 5: 0.1, 6: 0.2, 7: 0.2, '8 c=3': 0.2,
       '8 c=8': 0.2, 9: 0.2, 10: 0.05, 11: 0.1, 12: 0.05, 13: 0.2, 14: 0.05,
       15: 0.2, 16: 0.2, 17: 0.3, 18: 0.2, 19: 0.3}
STOP = {2: 0.0313, 5: 0.0359, 7: 0.0917, 11: 0.0401, 14: 0.02256, 15: 0.1274,
        18: 0.0507}

CASES = _cases()
BY_NAME = dict((c.name, c) for c in CASES)


def twin(name):
  """The first case of the same problem: the two split modes of a row share
  images, kernels and references."""
  base = name.replace(' bf16x3', ' f16x3')
  return base if base in BY_NAME else name


# one representative per family and split mode
OPTION_CASES = [c for c in CASES if c.stop_eps is not None]
OPTIONS = ('ista', 'warm', 'stop', 'nonneg', 'hard')


def padding(case):
  """((lead_v, trail_v), (lead_h, trail_h)) or None."""
  if case.pad != REF:
    return case.pad
  return tuple(sc_oracle.conv_padding_amount(case.image[i], case.kernel[i],
                                             case.stride[i]) for i in (0, 1))


def blank_axis(case):
  pad = padding(case)
  return pad is not None and (pad[0][1] == 0 or pad[1][1] == 0)


def geometry(case):
  pad = padding(case) or ((0, 0), (0, 0))
  return Geom(case.b, case.c, case.image[0] + sum(pad[0]),
              case.image[1] + sum(pad[1]), case.s, case.kernel[0],
              case.kernel[1], case.stride[0], case.stride[1],
              int(case.pad is not None), pad[0][0], pad[0][1], pad[1][0],
              pad[1][1])


def same_geometry(g, struct):
  """g against the vtc_conv_geometry utils.convolutions.geometry filled."""
  return all(getattr(struct, f) == getattr(g, f) for f in Geom._fields)


def sample_images(case):
  """The images that meet the oracle: all, or a seeded sorted sample that
  holds the first and the last."""
  if case.sample is None:
    return np.arange(case.b)
  rs = np.random.RandomState(9000 + CASES.index(BY_NAME[twin(case.name)]))
  inner = 1 + rs.choice(case.b - 2, size=case.sample - 2, replace=False)
  return np.sort(np.concatenate([[0], inner, [case.b - 1]]))


Problem = collections.namedtuple('Problem', 'case geom pad X D eta images')


@functools.lru_cache(maxsize=None)
def problem(name):
  """Images 0.5 N(0, 1) inside a zero frame, unit-norm kernels, and the
  convergent step 1 / (cover * lambda_max(F F^T)) of
  tests/test_large_batch_gpu.py."""
  case = BY_NAME[name]
  g, pad = geometry(case), padding(case)
  rs = np.random.RandomState(8000 + 10 * CASES.index(BY_NAME[twin(name)]))
  X = np.zeros((g.b, g.c, g.h, g.w), np.float32)
  (lv, tv), (lh, th) = pad or ((0, 0), (0, 0))
  X[:, :, lv:g.h - tv, lh:g.w - th] = (0.5 * rs.randn(
      g.b, g.c, g.h - lv - tv, g.w - lh - th)).astype(np.float32)
  D = rs.randn(g.s, g.c, g.kh, g.kw).astype(np.float32)
  D /= np.sqrt((D.astype(np.float64) ** 2).sum(axis=(1, 2, 3)))[
      :, None, None, None].astype(np.float32)
  eta = float(sc_oracle.conv_stepsize(torch.from_numpy(D).double())) / cover(g)
  return Problem(case, g, pad, X, D, eta, sample_images(case))


def oracle(p, dtype, num_iters, variant='fista', images=None, lam=None, **kw):
  X = p.X if images is None else p.X[images]
  return sc_oracle.conv_ista_fista(
      torch.from_numpy(X).to(dtype), torch.from_numpy(p.D).to(dtype),
      p.case.stride, p.pad, p.case.lam if lam is None else lam, num_iters,
      variant=variant, stepsize=p.eta, **kw)


def active_fraction(codes):
  return float((np.asarray(codes) != 0).mean())


def assert_input_conditions(p, ref64, ref32, what, tol=None, stop=None):
  """On the references alone: the case is not degenerate (a share of the code
  entries is non-zero, a share is not; blank-axis cases, whose codes are all
  zero, are exempt), the iterates did not grow, and float32 arithmetic
  reaches half the gate with no support flip above NEAR_THRESHOLD: the gate
  leaves room for the kernels' rounding and none for a wrong one.  stop =
  (mean steps of the float64 ISTA trace, iteration count): the mean step of
  the stopping iteration and of the one before it miss stop_eps by STOP_MARGIN
  of it."""
  if stop is not None:
    steps, count = stop
    eps = p.case.stop_eps
    assert 1 < count < STOP_ITERS, what
    assert steps[count - 1] <= (1 - STOP_MARGIN) * eps, what
    assert steps[count - 2] >= (1 + STOP_MARGIN) * eps, what
  frac = active_fraction(ref64)
  if blank_axis(p.case):
    assert frac == 0.0, what
  else:
    lo, hi = ACTIVE_BAND
    assert lo <= frac <= hi, '%s: %.3f of the codes non-zero' % (what, frac)
  peak = float(np.abs(ref64).max())
  assert peak < MAX_CODE, '%s: max |codes| %.3g' % (what, peak)
  err, _ = helpers.assert_codes_match(
      ref32, ref64, (gate(p.case.route)[0] if tol is None else tol) / 2,
      what + ': float32 oracle', max_flip_mag=helpers.NEAR_THRESHOLD)
  return frac, err


@functools.lru_cache(maxsize=None)
def reference(name, variant='fista', nonnegative_only=False):
  """(float64 codes, float32 codes) of the sampled images after T
  iterations."""
  if twin(name) != name:
    return reference(twin(name), variant, nonnegative_only)
  p = problem(name)
  return tuple(oracle(p, dtype, T, variant, p.images,
                      nonnegative_only=nonnegative_only).numpy()
               for dtype in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def warm_reference(name):
  """(initial codes of the whole batch as float32, float64 and float32 codes
  of the sampled images WARM_ITERS iterations later)."""
  if twin(name) != name:
    return warm_reference(twin(name))
  p = problem(name)
  init = oracle(p, torch.float64, WARM_FROM).float()
  refs = [oracle(p, dtype, WARM_ITERS, images=p.images,
                 initial_codes=init[p.images].to(dtype)).numpy()
          for dtype in (torch.float64, torch.float32)]
  return init.numpy(), refs[0], refs[1]


def _hard_oracle(p, dtype, eta):
  return sc_oracle.conv_ista_fista(
      torch.from_numpy(p.X[p.images]).to(dtype),
      torch.from_numpy(p.D).to(dtype), p.case.stride, p.pad, HARD_CUTOFF / eta,
      1, stepsize=eta, hard_threshold=True).numpy()


@functools.lru_cache(maxsize=None)
def hard_step(name):
  """The step of the hard-threshold run.  It is a single iteration, so the
  step need not be the convergent one: HARD_GATE was set at eta = 0.02 and
  lambda = 0.05, a cutoff of 1e-3 under codes of about 1e-2.  A flip at the
  cutoff costs cutoff / |codes| in relative error whatever the arithmetic;
  on the smaller problems here the step doubles, at the same cutoff, until
  one such flip costs at most a quarter of the relative gate."""
  if twin(name) != name:
    return hard_step(twin(name))
  p, eta = problem(name), HARD_ETA
  while HARD_GATE[1] / np.linalg.norm(_hard_oracle(p, torch.float64, eta)) > (
      HARD_GATE[0] / 4):
    eta *= 2
  return eta


def hard_lam(name):
  """The sparsity weight that keeps the cutoff lambda * eta of the
  hard-threshold run at HARD_CUTOFF, where HARD_GATE was set."""
  return HARD_CUTOFF / hard_step(name)


@functools.lru_cache(maxsize=None)
def hard_reference(name):
  """(float64 codes, float32 codes) after one iteration with a hard threshold
  (a discontinuous threshold turns last-bit differences into flips of the
  cutoff's size, which move their neighbours in later iterations;
  tests/test_conv_gpu.py)."""
  if twin(name) != name:
    return hard_reference(twin(name))
  p = problem(name)
  return tuple(_hard_oracle(p, dtype, hard_step(name))
               for dtype in (torch.float64, torch.float32))


@functools.lru_cache(maxsize=None)
def stop_trace(name):
  """Float64 ISTA on the whole batch: (codes after each iteration, mean step
  |c_k - c_(k-1)| / eta of each iteration), STOP_ITERS of them."""
  if twin(name) != name:
    return stop_trace(twin(name))
  p = problem(name)
  _, trace = oracle(p, torch.float64, STOP_ITERS, 'ista',
                    trace_at=set(range(1, STOP_ITERS + 1)))
  codes = [trace[k].numpy() for k in range(1, STOP_ITERS + 1)]
  steps, prev = [], np.zeros_like(codes[0])
  for c in codes:
    steps.append(float(np.mean(np.abs(c - prev) / p.eta)))
    prev = c
  return codes, steps


def stop_count(steps, eps):
  """Iterations an early-stopping run makes: the first k > 1 whose mean step
  is below eps."""
  for k in range(2, len(steps) + 1):
    if steps[k - 1] < eps:
      return k
  return len(steps)


@functools.lru_cache(maxsize=None)
def stop_reference(name):
  """Early stopping is a mean over the whole batch: the oracle runs on all of
  it.  Returns (float64 codes, float32 codes, iteration count).  The mean
  step of the stopping iteration and of the one before it both miss stop_eps
  by STOP_MARGIN of it: the device, which sums in another order and whose
  codes differ at the 1e-6 level, cannot stop elsewhere."""
  if twin(name) != name:
    return stop_reference(twin(name))
  p = problem(name)
  eps = p.case.stop_eps
  codes, steps = stop_trace(name)
  count = stop_count(steps, eps)
  assert 1 < count < STOP_ITERS, count
  assert steps[count - 1] <= (1 - STOP_MARGIN) * eps, (name, steps[count - 1])
  assert all(m >= (1 + STOP_MARGIN) * eps for m in steps[1:count - 1]), name
  ref32, trace32 = oracle(p, torch.float32, STOP_ITERS, 'ista',
                          early_stopping_epsilon=eps,
                          trace_at=set(range(1, STOP_ITERS + 1)))
  assert len(trace32) == count
  ref64 = oracle(p, torch.float64, STOP_ITERS, 'ista',
                 early_stopping_epsilon=eps)
  assert np.array_equal(ref64.numpy(), codes[count - 1])
  return codes[count - 1], ref32.numpy(), count


# ------------------------------------------------ float64 iteration with hooks
def iterate(p, num_iters=T, variant='fista', images=None, mask=None,
            synthesis=None, analysis_dictionary=None, after_prox=None,
            betas=None):
  """The float64 iteration of sc_oracle.conv_ista_fista on the sampled images,
  its pieces replaceable (tests/test_conv_gates_host.py):
  mask: the (1, 1, H, W) mask; synthesis(y, D) -> reconstruction;
  analysis_dictionary: the kernels the analysis correlates with;
  after_prox(codes, previous codes) -> codes; betas: the momentum weights."""
  images = p.images if images is None else images
  X = torch.from_numpy(p.X[images]).double()
  D = torch.from_numpy(p.D).double()
  Da = D if analysis_dictionary is None else analysis_dictionary
  if mask is None:
    mask = sc_oracle.conv_mask(X[:1], p.pad)
  if synthesis is None:
    synthesis = lambda y, D: sc_oracle.conv_synthesis(y, D, p.case.stride)
  if betas is None:
    betas = sc_oracle.fista_betas(num_iters)
  cutoff = p.case.lam * p.eta
  ch, cw = code_dims(p.geom)
  c_prev = X.new_zeros(len(images), p.geom.s, ch, cw)
  y = c_prev.clone()
  for k in range(num_iters):
    r = mask * (synthesis(y, D) - X)
    c = sc_oracle.shrink_(
        y - p.eta * sc_oracle.conv_analysis(r, Da, p.case.stride), cutoff)
    if after_prox is not None:
      c = after_prox(c, c_prev)
    y = c + betas[k] * (c - c_prev) if variant == 'fista' else c
    c_prev = c
  return c_prev.numpy()
