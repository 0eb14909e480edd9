"""The fence table of tests/test_abi_fences_gpu.py on pointers that are only
element-aligned.

include/vtc_hip.h (Conventions) promises that a data pointer needs no more than
the alignment of its element.  Ordinary callers rely on that: a minibatch
slice `patches[k:]` of 7x7 patches, `images[k:]` of 70x93 images, a dictionary
kept inside a larger parameter buffer.  The fence table itself runs on
payloads that are at least 256-byte aligned, so every 16-byte route of the
library passes its alignment gate there; here every case of the table runs
again with

  one at a time   each non-null pointer in turn one element off a 16-byte
                  boundary (4 bytes for float32 / int32, 8 for float64, 1, 2 or
                  3 for the byte tables), all others aligned: a gate that ORs
                  some pointers and forgets one shows only when the forgotten
                  one alone is skewed;
  all together    every payload 8 bytes off, then every payload 12 bytes off
                  (the nearest multiple of the element size).

The workspace is fenced, poisoned, of exactly the queried size and NOT skewed
(the header asks 256-byte alignment for it).  Every call must return VTC_OK --
or VTC_ERR_UNSUPPORTED where the header allows it: VTC_BF16 of
vtc_fc_ista_fista(_dev), which exists only as the fused 16-byte kernel -- and

  on VTC_OK           every guard intact, inputs bitwise unchanged, every
                      floating-point output fully written, and the result
                      within the case's own bounds of its float64 truth (never
                      compared with the aligned call: a fallback route may
                      round differently);
  on the refusal      outputs and workspace untouched, inputs unchanged, the
                      error text names the skewed argument.

profiles/pointer_alignment.txt holds the audit behind the gates and the list
of refusals.
"""
import ctypes
import re
import time

import numpy as np
import pytest
import torch

import fences
import test_abi_fences_gpu as table

pytestmark = pytest.mark.gpu

OK, ERR_UNSUPPORTED = 0, 2

# entry points the header's alignment paragraph lists, and the cases of the
# table that ask them for the precision it names (VTC_BF16)
MAY_REFUSE = ('vtc_fc_ista_fista', 'vtc_fc_ista_fista_dev')
# the argument names of the header for the table's input / output keys
ARGUMENT = {'initial': 'initial_codes'}

# order in which a refusal looks for the first unaligned pointer
# (csrc/fc_inference.hip)
ARGUMENT_ORDER = ('images', 'dictionary', 'initial', 'codes')

_wall = {'calls': 0, 'cases': 0, 'refused': [], 'seconds': 0.0}


def _expected_refusals():
  """Every (case id, label) of the skewed table that must be refused --
  profiles/pointer_alignment.txt lists the same: the VTC_BF16 rows, each
  16-byte-gated pointer alone and the two all-together calls; a skewed
  step-size pointer is no refusal."""
  out = set()
  for c in table.CASES:
    if not _may_refuse(c):
      continue
    out.add((c.id, 'all +8'))
    out.add((c.id, 'all +12'))
    for name in ARGUMENT_ORDER:
      if name != 'initial' or 'warm' in c.branch:
        out.add((c.id, '%s +4' % name))
  return out


def _may_refuse(c):
  return c.entry in MAY_REFUSE and '-bf16-' in c.id


def _torch_dtype(np_dtype):
  return torch.from_numpy(np.zeros(1, np_dtype)).dtype


def _pointers(spec):
  """(name, element size) of every non-null data pointer of the case."""
  out = []
  for k, v in spec.inputs.items():
    if v is not None:
      out.append((k, np.asarray(v).dtype.itemsize))
  for k, shape_dtype in spec.outputs.items():
    if shape_dtype is not None:
      out.append((k, np.dtype(shape_dtype[1]).itemsize))
  return out


def _skewed_call(device, lib, stream, c, spec, skews, label):
  """One fenced call with payload `k` starting skews[k] bytes off."""
  what = '%s [%s]' % (c.id, label)
  t, f = {}, {}
  for k, v in spec.inputs.items():
    if v is None:
      t[k] = None
    else:
      t[k], f[k] = fences.fenced_copy(v, device, skew=skews.get(k, 0))
  for k, shape_dtype in spec.outputs.items():
    if shape_dtype is None:
      t[k] = None
      continue
    shape, dtype = shape_dtype
    t[k], f[k] = fences.fenced(shape, _torch_dtype(dtype), device,
                               skew=skews.get(k, 0))
  for k, fence in f.items():
    if fence.nbytes:
      assert t[k].data_ptr() % 16 == skews.get(k, 0), (what, k)
      assert t[k].is_contiguous()
  ws_ptr = ctypes.c_void_p(0)
  if spec.ws_bytes > 0:
    ws, f['workspace'] = fences.fenced_workspace(spec.ws_bytes, device)
    assert ws.data_ptr() % 256 == 0
    ws_ptr = table._p(ws)
  rc = spec.call(lib, {k: table._p(v) for k, v in t.items()}, ws_ptr,
                 spec.ws_bytes, stream)
  torch.cuda.synchronize(device)
  _wall['calls'] += 1
  text = lib.vtc_last_error().decode()
  for k, fence in f.items():
    fence.assert_intact('%s: %s' % (what, k))

  def inputs_unchanged(names):
    for k in names:
      v = spec.inputs[k]
      if v is not None:
        assert torch.equal(t[k].cpu(), torch.from_numpy(
            np.ascontiguousarray(v)).reshape(t[k].shape)), (
                '%s: input %s was modified' % (what, k))

  if rc == ERR_UNSUPPORTED:
    assert _may_refuse(c), '%s: refused (%s)' % (what, text)
    inputs_unchanged(list(spec.inputs))
    for k, fence in f.items():
      if k in spec.outputs or k == 'workspace':
        fence.assert_untouched('%s (refused): %s' % (what, k))
    # the text names, as a whole word, the first skewed argument in the
    # order the call checks them: for a one-at-a-time call THE skewed one
    first = [k for k in ARGUMENT_ORDER if skews.get(k, 0)][0]
    words = re.findall(r'[A-Za-z_]+', text)
    assert ARGUMENT.get(first, first) in words, (
        '%s: the refusal "%s" does not name %s' % (what, text, first))
    for k in ARGUMENT_ORDER:
      if k != first:
        assert ARGUMENT.get(k, k) not in words, (what, text)
    assert '16-byte' in text, text
    _wall['refused'].append((c.id, label))
    return

  assert rc == OK, '%s: status %d (%s)' % (what, rc, text)
  inputs_unchanged([k for k in spec.inputs if k not in spec.inout])
  names = [k for k, v in spec.outputs.items() if v is not None]
  got = {k: t[k] for k in names + list(spec.inout)}
  for k, v in got.items():
    if v.dtype.is_floating_point:
      f[k].assert_written('%s: %s' % (what, k))
  for item, err, bound in spec.truth({k: table._np(v) for k, v in got.items()},
                                     dict(spec.inputs)):
    print('skewed %-60s %-14s err %.3e bound %.3e' % (what, item, err, bound))
    assert err <= bound, '%s %s: %.3e > %.3e' % (what, item, err, bound)


def run_skewed(device, c):
  import vtc_hip
  lib = table._lib()
  spec = c.make(lib)
  if spec.route is not None:
    spec.route(lib)
  stream = vtc_hip.current_stream(device)
  start = time.perf_counter()
  pointers = _pointers(spec)
  bytes_seen = 0
  for name, itemsize in pointers:
    skew = itemsize
    if itemsize == 1:                 # byte tables: 1, 2, 3 bytes in turn
      skew = 1 + bytes_seen % 3
      bytes_seen += 1
    _skewed_call(device, lib, stream, c, spec, {name: skew},
                 '%s +%d' % (name, skew))
  for want in (8, 12):
    skews = {name: fences.skew_for(itemsize, want)
             for name, itemsize in pointers}
    _skewed_call(device, lib, stream, c, spec, skews, 'all +%d' % want)
  _wall['seconds'] += time.perf_counter() - start
  _wall['cases'] += 1


@pytest.mark.parametrize('c', table.CASES, ids=[c.id for c in table.CASES])
def test_skewed_call(device, c):
  run_skewed(device, c)


def test_refusals_are_the_listed_ones(device):
  """Runs after the table (same module, file order): the skewed calls that
  were refused are VTC_BF16 inference calls, nothing else, and there are some
  (the refusal path is exercised)."""
  print('skewed_fence_summary calls %d refused %d seconds %.1f'
        % (_wall['calls'], len(_wall['refused']), _wall['seconds']))
  for what in _wall['refused']:
    print('skewed_fence_refused %s [%s]' % what)
  expected = _expected_refusals()
  assert len(expected) == 64      # the figure of profiles/pointer_alignment.txt
  refused = set(_wall['refused'])
  assert len(refused) == len(_wall['refused'])
  assert refused <= expected, sorted(refused - expected)
  if _wall['cases'] == len(table.CASES):     # the whole table ran before us
    assert refused == expected, sorted(expected - refused)
