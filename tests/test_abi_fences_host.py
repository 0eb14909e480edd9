"""The fence table of tests/test_abi_fences_gpu.py covers the whole C ABI, and
the fences of tests/fences.py bite.  No GPU needed."""
import pathlib
import re

import fences
import helpers
import test_abi_fences_gpu as table

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'vtc_hip.h'

# entry points that write no device memory of the caller's, with the reason
EXEMPT = {
    'vtc_draw_patch_positions': 'host only: no device work, host arrays',
    'vtc_conv_code_dims': 'host only: two host integers',
    'vtc_last_error': 'returns a string',
    'vtc_version': 'returns a string',
    'vtc_abi_version': 'returns an integer',
    'vtc_init': 'no arguments; places the library\'s own constants',
}


def declarations():
  """name -> argument text of every function include/vtc_hip.h declares."""
  text = HEADER.read_text()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  return {m.group(1): m.group(2)
          for m in re.finditer(r'\b(vtc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', text)}


def needs_a_fence(args):
  """Takes a workspace or at least one pointer it may write through."""
  for arg in args.split(','):
    arg = ' '.join(arg.split())
    if '*' not in arg:
      continue
    if 'workspace' in arg or not arg.startswith('const '):
      return True
  return False


def test_header_is_parsed():
  decl = declarations()
  assert len(decl) >= 50
  assert needs_a_fence(decl['vtc_gram'])
  assert needs_a_fence(decl['vtc_fc_ista_fista'])
  assert not needs_a_fence(decl['vtc_conv_x3_supported'])
  assert not needs_a_fence(decl['vtc_lambda_max_workspace_bytes'])


def test_every_writing_entry_point_has_a_fenced_case():
  decl = declarations()
  fenced = set(c.entry for c in table.CASES)
  assert fenced <= set(decl), sorted(fenced - set(decl))
  missing = [name for name, args in sorted(decl.items())
             if needs_a_fence(args) and name not in fenced
             and name not in EXEMPT]
  assert not missing, 'no fenced case for: ' + ', '.join(missing)
  for name in EXEMPT:
    assert name in decl and name not in fenced, name


def test_case_ids_are_unique_and_name_their_branch():
  ids = [c.id for c in table.CASES]
  assert len(ids) == len(set(ids))
  for c in table.CASES:
    assert c.branch and c.entry.startswith('vtc_'), c.id


def test_no_row_of_the_table_was_dropped():
  """tests/golden/abi_fence_ids.txt lists every row; the table must be that
  set exactly, so a deleted (or an unrecorded) row is reported by name."""
  listed = (helpers.GOLDEN / 'abi_fence_ids.txt').read_text().split()
  assert len(listed) == len(set(listed))
  ids = set(c.id for c in table.CASES)
  missing = sorted(set(listed) - ids)
  assert not missing, 'rows dropped from the fence table: ' + ', '.join(missing)
  unlisted = sorted(ids - set(listed))
  assert not unlisted, ('rows not recorded in tests/golden/abi_fence_ids.txt: '
                        + ', '.join(unlisted))


def test_every_inference_route_runs_at_every_batch_size():
  ids = set(c.id for c in table.CASES)
  for b in table.BATCHES:
    for stem in ('fc_small-s64', 'chip16-144x576', 'fused-s512-f16x3',
                 'stream-s1280-f16x3', 'tiled-f32-100x200'):
      assert 'fc_ista_fista-%s-b%d' % (stem, b) in ids
      assert 'fc_ista_fista_dev-dev-%s-b%d' % (stem, b) in ids
    for s in (256, 512, 1024):
      for prec in ('f16x3', 'bf16x3', 'bf16'):
        assert 'fc_ista_fista-fused-s%d-%s-b%d' % (s, prec, b) in ids


def test_fences_report_each_deliberate_fault():
  reports = fences.self_test('cpu')
  assert len(reports) == 3
  assert 'trailing guard' in reports[0] and 'first 0 past the end' in reports[0]
  assert 'leading guard' in reports[1] and 'nearest 1 before' in reports[1]
  assert 'not written' in reports[2] and 'index 17' in reports[2]


def test_skewed_fences_report_each_deliberate_fault():
  """A payload that starts 1 to 12 bytes past the aligned position keeps both
  guards against its first and last byte: one damaged byte on either side is
  seen at the right offset, and so is an element left unwritten."""
  found = fences.self_test_skewed('cpu')
  assert sorted(found) == [('float32', 4), ('float32', 8), ('float32', 12),
                           ('float64', 8), ('int32', 4), ('uint8', 1),
                           ('uint8', 2), ('uint8', 3)]
  for (dtype, skew), (past, before, unwritten) in found.items():
    assert 'trailing guard, 1 bytes damaged, first 0 past the end' in past
    assert 'leading guard, 1 bytes damaged, nearest 1 before' in before
    if dtype.startswith('float'):
      assert 'not written' in unwritten and 'index 17' in unwritten
    else:
      assert unwritten is None


def test_skew_zero_is_the_old_layout():
  import torch
  f = fences.Fence((5, 7), torch.float32, 'cpu')
  assert f.skew == 0 and f.lead == f.guard
  assert f.flat.numel() == 2 * f.guard + f.nbytes
  assert f.payload.data_ptr() == f.flat.data_ptr() + f.guard


def test_guard_length_rule():
  for nbytes in (0, 1, 511, 1 << 20, (1 << 20) + 1, 5 << 20):
    g = fences.guard_bytes(nbytes)
    assert g % 512 == 0 and g >= max(1 << 20, nbytes)
