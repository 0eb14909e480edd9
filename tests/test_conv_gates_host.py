"""CPU checks behind tests/test_conv_routes_gpu.py: the dispatch mirror gives
every case of the table its named route at 256 CUs and the table holds every
branch it was built for; the mirror turns where the C dispatch turns; every
case's input conditions hold on the references alone; the float64 iteration
with replaceable pieces (conv_routes_data.iterate) agrees with sc_oracle; and
the gates of the route tests notice what these kernels can get wrong -- each
fault below, carried through all T iterations of the float64 iteration of a
named case, fails helpers.assert_codes_match at that case's gate.  No GPU
needed."""
import numpy as np
import pytest
import torch

import conv_routes_data as crd
import helpers
import sc_oracle

CUS = 256      # MI355X

IDS = [c.name for c in crd.CASES]


def _geom(b, c, ch, cw, s, kh, kw, sv=1, sh=1):
  """A geometry from its code map."""
  return crd.Geom(b, c, (ch - 1) * sv + kh, (cw - 1) * sh + kw, s, kh, kw, sv,
                  sh, 0, 0, 0, 0, 0)


@pytest.mark.parametrize('case', crd.CASES, ids=IDS)
def test_dispatch_mirror_names_each_case(case):
  g = crd.geometry(case)
  assert crd.conv_route(g, case.precision, CUS) == case.route
  ch, cw = crd.code_dims(g)
  assert (ch - 1) * g.stride_v + g.kh == g.h      # make_geo accepts it
  assert (cw - 1) * g.stride_h + g.kw == g.w
  number = case.name.split()[0]
  # the sizes that put the case on its branch
  if case.route[0] == 'x3-fused':
    assert g.c == 1 and g.s > 32 and g.kh <= 11
  if number == '3':
    assert 2 * crd.x3_slots(11) * (208 + 8) * 2 > 100 * 1024 >= (
        2 * crd.x3_slots(11) * (112 + 8) * 2)      # two chunks of 112
  if number == '4':
    assert ch % 8 and cw % 32 and ch > 8 and cw > 32
  if number == '6':
    assert g.s < 32      # 'auto' never takes a split route here
  if number == '10':
    plan = crd.x3_plan(g, CUS)
    assert plan.blocks8 == 16 * CUS
    assert 0 in crd.sample_images(case) and g.b - 1 in crd.sample_images(case)
    assert len(set(crd.sample_images(case))) == 8
  if number == '11':
    assert crd.unit_groups(g, 1) == (3, 16) and g.s % 16       # 16 + 16 + 8
    assert g.h <= crd.UNIT_TY and g.w <= crd.UNIT_TX
  if number == '12':
    assert (g.h, g.w) == (36, 36) and (ch, cw) == (32, 32)
  if number == '13':
    assert g.h % crd.UNIT_TY and g.w % crd.UNIT_TX and g.h > crd.UNIT_TY
  if number == '14':
    assert crd.unit_geometry(g) and not crd.unit_analysis_fits(g)
    assert crd.unit_analysis_bytes(g) == 146112
  if number == '15':
    assert crd.cover(g) > 16 and g.stride_v != g.stride_h and g.kh != g.kw
    assert ch > 16 and cw > 16 and ch % 16 and cw % 16
  if number == '16':
    assert g.c * 43 * 43 * 4 > 40 * 1024 >= crd.plan_analysis(g)[2]
    assert ch % 8 and cw % 16
  if case.route[0] == 'patch':
    assert crd.cover(g) <= 16


def test_case_table_covers_every_branch():
  routes = [c.route for c in crd.CASES]
  split = [r for r in routes if r[0].startswith('x3')]
  f32 = [r for r in routes if not r[0].startswith('x3')]
  for fam in ('x3-fused', 'x3-two'):
    assert set(r[1] for r in split if r[0] == fam) == {'f16', 'bf16'}
  assert set(r[2] for r in split) == {32, 64}                       # AC
  assert any(r[2] == 32 and c.s > 32 for r, c in zip(routes, crd.CASES)
             if r[0] == 'x3-two')
  # chunks 1 and more, ragged and not
  assert {(r[3] > 1, r[4]) for r in split} >= {(False, False), (False, True),
                                                (True, True)}
  assert any(r[5] > 1 and c.kernel == (11, 11)
             for r, c in zip(routes, crd.CASES) if r[0] == 'x3-fused')
  assert any(r[5] > 1 and c.kernel == (16, 16)
             for r, c in zip(routes, crd.CASES) if r[0] == 'x3-two')
  assert set(r[6] for r in split) == {1, 2, 4}                      # ana_shift
  assert set(r[7] for r in split) == {4, 8}                         # ana_rows
  assert set(r[0] for r in f32) == {'patch', 'unit', 'unit-synth+direct',
                                    'direct'}
  assert any(r[0] == 'unit' and r[1] > 1 for r in f32)
  assert any(r[0] == 'unit' and r[1] != r[2] for r in f32)
  assert any(r[0] == 'direct' and r[3] != (16, 16) for r in f32)
  # per family: a blank-axis mask and an asymmetric one; one case unmasked
  for fam in ('x3-fused', 'x3-two', 'unit', 'direct', 'patch'):
    pads = [crd.padding(c) for c in crd.CASES if crd.family(c.route) == fam]
    assert any(p and (p[0][1] == 0 or p[1][1] == 0) for p in pads), fam
    assert any(p and p[0][0] != p[0][1] and p[1][0] != p[1][1] and
               0 not in (p[0][1], p[1][1]) for p in pads), fam
  assert sum(c.pad is None for c in crd.CASES) == 1
  # the representatives of the options test: cases 2, 5, 7, 11, 14, 15, 18
  assert sorted(set(int(c.name.split()[0]) for c in crd.OPTION_CASES)) == [
      2, 5, 7, 11, 14, 15, 18]


def test_dispatch_mirror_boundaries():
  route = crd.conv_route
  # cover 16 / 17: the patch contraction gives way to the direct kernels
  assert crd.cover(_geom(2, 1, 5, 5, 4, 16, 3, 1, 3)) == 16
  assert route(_geom(2, 1, 5, 5, 4, 16, 3, 1, 3), 'f32', CUS)[0] == 'patch'
  assert crd.cover(_geom(2, 1, 5, 5, 4, 17, 3, 1, 3)) == 17
  assert route(_geom(2, 1, 5, 5, 4, 17, 3, 1, 3), 'f32', CUS)[0] == 'direct'
  # stride 1 is never a patch geometry
  assert route(_geom(2, 1, 5, 5, 4, 3, 3), 'f32', CUS)[0] == 'direct'
  # s 32 / 33: atoms per analysis block, and with them the fused kernel
  assert route(_geom(2, 1, 20, 20, 32, 5, 5), 'f16x3', CUS)[:4] == (
      'x3-two', 'f16', 32, 1)
  assert route(_geom(2, 1, 20, 20, 33, 5, 5), 'f16x3', CUS)[:5] == (
      'x3-fused', 'f16', 64, 1, True)
  # s 64 / 65: a second chunk
  assert route(_geom(2, 1, 20, 20, 64, 5, 5), 'bf16x3', CUS)[2:5] == (
      64, 1, False)
  assert route(_geom(2, 1, 20, 20, 65, 5, 5), 'bf16x3', CUS)[2:5] == (
      64, 2, True)
  # the fused kernel: one channel, kernels up to 11 x 11
  assert route(_geom(2, 1, 20, 20, 64, 11, 11), 'f16x3', CUS)[0] == 'x3-fused'
  assert route(_geom(2, 1, 20, 20, 64, 16, 16), 'f16x3', CUS)[0] == 'x3-two'
  assert route(_geom(2, 2, 20, 20, 64, 5, 5), 'f16x3', CUS)[0] == 'x3-two'
  # ... and fragment-order maps below 2^32 bytes (8 x 32 items of 64 KiB)
  assert route(_geom(4095, 1, 16, 128, 64, 5, 5), 'f16x3', CUS)[0] == (
      'x3-fused')
  assert route(_geom(8192, 1, 16, 128, 64, 5, 5), 'f16x3', CUS)[0] == 'x3-two'
  # synthesis planes of 11 x 11 kernels, 640 bytes per atom and 16 atoms at a
  # time: one chunk up to 144 atoms
  assert route(_geom(1, 1, 20, 20, 144, 11, 11), 'f16x3', CUS)[5] == 1
  assert route(_geom(1, 1, 20, 20, 145, 11, 11), 'f16x3', CUS)[5] == 2
  # blocks8 at 16 * CUs and one below: analysis blocks of 8 code rows
  for b, rows in ((2048, 8), (2047, 4)):
    g = _geom(b, 1, 16, 8, 32, 5, 5)
    assert crd.x3_plan(g, CUS).blocks8 == 2 * b
    assert route(g, 'f16x3', CUS)[7] == rows
  assert route(_geom(2048, 1, 16, 8, 32, 5, 5), 'f16x3', CUS + 1)[7] == 4
  # the 140 KiB edge of unit_analysis_fits: 16 x 16 kernels, one channel
  fits, over = _geom(1, 1, 20, 20, 125, 16, 16), _geom(1, 1, 20, 20, 126, 16,
                                                        16)
  assert crd.unit_analysis_bytes(fits) <= 140 * 1024 < (
      crd.unit_analysis_bytes(over))
  assert route(fits, 'f32', CUS)[0] == 'unit'
  assert route(over, 'f32', CUS) == ('unit-synth+direct', 1, 1, (16, 16))
  # the 40 KiB edge of plan_analysis: 22 x 22 windows of 7 x 7 kernels
  assert crd.plan_analysis(_geom(1, 21, 20, 20, 4, 7, 7)) == (16, 16, 40656)
  assert crd.plan_analysis(_geom(1, 22, 20, 20, 4, 7, 7))[:2] == (8, 16)
  assert route(_geom(1, 22, 20, 20, 4, 7, 7), 'f32', CUS) == (
      'direct', 1, 1, (8, 16))
  # the shrinking alternates between the axes, down to one position
  assert crd.plan_analysis(_geom(1, 32, 20, 20, 4, 13, 13, 2, 2))[:2] == (2, 4)
  assert crd.plan_analysis(_geom(1, 64, 20, 20, 4, 13, 13, 2, 2)) == (
      1, 1, 64 * 13 * 13 * 4)
  # unit groups: never more than ceil(s / 16), never more than 8, and fewer
  # once tiles * b passes 1536 / groups
  assert crd.unit_groups(_geom(1, 1, 20, 20, 9, 5, 5), 1) == (1, 12)
  assert crd.unit_groups(_geom(1, 1, 20, 20, 208, 5, 5), 1)[0] == 8
  assert crd.unit_groups(_geom(511, 1, 32, 32, 64, 5, 5), 1) == (4, 16)
  assert crd.unit_groups(_geom(512, 1, 32, 32, 64, 5, 5), 1) == (3, 24)
  # 'auto': the f16 split from 32 kernels on, soft thresholds only
  g = _geom(2, 1, 20, 20, 32, 5, 5)
  assert crd.resolve_precision('auto', g, False, True) == 'f16x3'
  assert crd.resolve_precision('auto', g, True, True) == 'f32'
  assert crd.resolve_precision('auto', g, False, False) == 'f32'
  assert crd.resolve_precision('auto', g._replace(s=31), False, True) == 'f32'
  assert crd.resolve_precision('bf16x3', g._replace(s=4), True, True) == (
      'bf16x3')
  # geometries without a split form
  assert crd.x3_plan(_geom(2, 1, 20, 20, 32, 7, 7), CUS) is None
  assert crd.x3_plan(_geom(2, 9, 20, 20, 32, 5, 5), CUS) is None
  assert crd.x3_plan(_geom(2, 1, 20, 20, 32, 8, 8, 2, 2), CUS) is None


@pytest.mark.parametrize('case', crd.CASES, ids=IDS)
def test_input_conditions_hold_on_the_references(case):
  """What the GPU tests assert before they look at device output, here for
  every case and option."""
  p = crd.problem(case.name)
  ref64, ref32 = crd.reference(case.name)
  frac, err = crd.assert_input_conditions(p, ref64, ref32, case.name)
  print('%-40s fista  active %.3f  float32 oracle %.1e  max %.3g' % (
      case.name, frac, err, np.abs(ref64).max()))
  if case.sample is not None:
    # images are independent: the sampled oracle is the whole batch's
    few = p.images[:2]
    assert np.array_equal(
        crd.oracle(p, torch.float64, crd.T, images=few).numpy(), ref64[:2])
  if case.stop_eps is None:
    return
  for what, refs in (('ista', crd.reference(case.name, 'ista')),
                     ('nonneg', crd.reference(case.name, 'fista', True)),
                     ('warm', crd.warm_reference(case.name)[1:]),
                     ('stop', crd.stop_reference(case.name)[:2])):
    stop = (crd.stop_trace(case.name)[1],
            crd.stop_reference(case.name)[2]) if what == 'stop' else None
    frac, err = crd.assert_input_conditions(p, refs[0], refs[1],
                                            case.name + ' ' + what, stop=stop)
    print('%-40s %-6s active %.3f  float32 oracle %.1e' % (
        case.name, what, frac, err))
  count = crd.stop_reference(case.name)[2]
  steps = crd.stop_trace(case.name)[1]
  print('%-40s stops after %d: mean steps %.4g, %.4g around eps %.4g' % (
      case.name, count, steps[count - 2], steps[count - 1], case.stop_eps))
  assert 1 < count < crd.STOP_ITERS
  assert steps[count - 2] >= (1 + crd.STOP_MARGIN) * case.stop_eps
  assert steps[count - 1] <= (1 - crd.STOP_MARGIN) * case.stop_eps
  hard64, hard32 = crd.hard_reference(case.name)
  assert 0.0 < crd.active_fraction(hard64) < 1.0
  assert abs(crd.hard_lam(case.name) * crd.hard_step(case.name) -
             crd.HARD_CUTOFF) < 1e-12
  # one flip at the cutoff fits a quarter of the relative gate
  assert crd.HARD_GATE[1] / np.linalg.norm(hard64) <= crd.HARD_GATE[0] / 4
  print('%-40s hard   active %.3f  step %.2f  |codes| %.2f' % (
      case.name, crd.active_fraction(hard64), crd.hard_step(case.name),
      np.linalg.norm(hard64)))
  helpers.assert_codes_match(hard32, hard64, crd.HARD_GATE[0] / 2,
                             case.name + ' hard',
                             max_flip_mag=crd.HARD_GATE[1])


@pytest.mark.parametrize('name', ['4 fused k=8 ragged items f16x3',
                                  '15 direct strided non-square',
                                  '17 direct stride 1 k=7 no padding',
                                  '22 unit blank columns'])
@pytest.mark.parametrize('variant', ['fista', 'ista'])
def test_iteration_matches_oracle(name, variant):
  p = crd.problem(name)
  ref = crd.oracle(p, torch.float64, crd.T, variant, p.images).numpy()
  ours = crd.iterate(p, crd.T, variant)
  if crd.blank_axis(p.case):
    assert not ours.any() and not ref.any()
  else:
    assert helpers.rel_err(ours, ref) < 1e-13


# ------------------------------------------------------------------- faults
def _synthesis_without(p, atoms, region=None):
  """The synthesis with the contribution of `atoms` (a slice) missing, in the
  whole image or in region = (image, rows, columns) only."""
  def synthesis(y, D):
    full = sc_oracle.conv_synthesis(y, D, p.case.stride)
    part = sc_oracle.conv_synthesis(y[:, atoms], D[atoms], p.case.stride)
    if region is None:
      return full - part
    img, rows, cols = region
    out = full.clone()
    out[img, :, rows, cols] -= part[img, :, rows, cols]
    return out
  return synthesis


def _fault_chunk_dropped():
  # the second 64-atom chunk of the fused kernel never reaches one item's
  # 18 x 42 partial tile
  p = crd.problem('2 fused ragged chunk f16x3')
  return p, crd.iterate(p, synthesis=_synthesis_without(
      p, slice(64, None), (0, slice(8, 26), slice(0, 42))))


def _fault_ragged_chunk_zeroed():
  p = crd.problem('2 fused ragged chunk f16x3')
  def after(c, c_prev):
    c = c.clone()
    c[:, 64:] = 0
    return c
  return p, crd.iterate(p, after_prox=after)


def _fault_stale_item_column():
  # the last column of one 8 x 32 item keeps its previous iterate
  p = crd.problem('4 fused k=8 ragged items f16x3')
  def after(c, c_prev):
    c = c.clone()
    c[1, :, 8:16, 31] = c_prev[1, :, 8:16, 31]
    return c
  return p, crd.iterate(p, after_prox=after)


def _fault_mask_shifted():
  p = crd.problem('13 unit c=3 ragged tiles')
  X = torch.from_numpy(p.X[:1]).double()
  return p, crd.iterate(p, mask=torch.roll(sc_oracle.conv_mask(X, p.pad), 1,
                                           dims=2))


def _fault_trail_zero_not_blank():
  # trail = 0 read as "no trailing frame" instead of the reference's `-0:`
  p = crd.problem('22 unit blank columns')
  (lv, tv), (lh, th) = p.pad
  assert th == 0 and tv > 0
  mask = torch.ones(1, 1, p.geom.h, p.geom.w, dtype=torch.float64)
  mask[:, :, :lv] = 0
  mask[:, :, p.geom.h - tv:] = 0
  mask[:, :, :, :lh] = 0
  return p, crd.iterate(p, mask=mask)


def _fault_taps_exchanged():
  # the analysis reads tap (dy, dx) of an 11 x 13 kernel at dx * 11 + dy
  p = crd.problem('15 direct strided non-square')
  D = torch.from_numpy(p.D).double()
  s, c, kh, kw = D.shape
  assert kh != kw
  swapped = D.reshape(s, c, kw, kh).transpose(2, 3).contiguous()
  return p, crd.iterate(p, analysis_dictionary=swapped)


def _fault_partial_synthesis_omitted():
  # the analysis sums two of the three partial syntheses: kernels 32 .. 39,
  # the partial last group, are missing from the residual
  p = crd.problem('11 unit 3 groups')
  return p, crd.iterate(p, synthesis=_synthesis_without(p, slice(32, None)))


def _fault_previous_beta():
  p = crd.problem('14 unit synthesis, direct analysis')
  betas = sc_oracle.fista_betas(crd.T)
  return p, crd.iterate(p, betas=[0.0] + betas[:-1])


FAULTS = {
    'a chunk dropped from the synthesis': _fault_chunk_dropped,
    'b ragged chunk zeroed': _fault_ragged_chunk_zeroed,
    'c stale last column of an item': _fault_stale_item_column,
    'd mask shifted by one row': _fault_mask_shifted,
    'e trail 0 does not blank': _fault_trail_zero_not_blank,
    'f dy and dx exchanged': _fault_taps_exchanged,
    'g partial synthesis omitted': _fault_partial_synthesis_omitted,
    'h beta of the previous iteration': _fault_previous_beta,
}


@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_gates_catch_kernel_faults(fault):
  p, codes = FAULTS[fault]()
  name = p.case.name
  tol, flip = crd.gate(p.case.route)
  ref64, ref32 = crd.reference(name)
  crd.assert_input_conditions(p, ref64, ref32, name)
  # the sound iteration passes, as float32
  helpers.assert_codes_match(crd.iterate(p).astype(np.float32), ref64, tol,
                             name, max_flip_mag=flip)
  bad = codes.astype(np.float32)
  flips = (bad != 0) != (ref64 != 0)
  worst = np.maximum(np.abs(bad), np.abs(ref64))[flips].max() if (
      flips.any()) else 0.0
  err = (helpers.rel_err(bad, ref64) if ref64.any() else
         float(np.abs(bad).max()))
  print('%-40s %-36s %s %.2e (gate %.0e)  largest flip %.1e' % (
      name, fault, 'rel' if ref64.any() else 'max', err, tol, worst))
  with pytest.raises(AssertionError):
    helpers.assert_codes_match(bad, ref64, tol, fault, max_flip_mag=flip)
