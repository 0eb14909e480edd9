"""
`utils.quantization` with the vector quantiser of the experiment's "Mod2" and
"Mod3" variants (experiments/rate_distortion_sparse_coding.py:600-840): a few
dozen coefficients of a sparse code go through scalar quantisers, the sparse
tail (23 of 64 coefficients there) is quantised as one vector by an
entropy-constrained vector quantiser fitted on the device.  The module is a
superset of utils.quantization, so the experiment needs one changed line:

  from utils import vector_quantization as quantization

The hot paths are the kernels of csrc/vq.hip behind include/vtc_vq.h
(DESIGN.md 4.16); device tensors in, device tensors out.

Codebooks of more than 4096 codewords.  include/vtc_vq.h stops at
VQ_MAX_CODEWORDS = 4096 and every default here stops there with it.  The
keyword max_codewords (vec_max_codewords in the R-D points), at most
VQ_LARGE_MAX_CODEWORDS = 131072, raises the limit: a codebook of kmax <= 4096
slots goes through the same entry points as ever, one of 4096 < kmax <=
max_codewords through their twins of include/vtc_vq_large.h (csrc/vq_large.hip,
DESIGN.md 4.20), which return the same bits where both apply, and a larger one
raises NotImplementedError naming the limit in force.  Index coding stops at
4096 symbols: source_code 'huffman' and 'ans' need a vector codebook of at most
4096 slots, which trim_vector_codebook makes of a fit that ended there.
source_code 'ans_split' codes the vector index under the split range coder of
include/ext/vtc_index_ans_split.h instead, whatever the codebook's size.
Which coder codes the scalar columns and which the vector column, in one
stream set or two, is the table _MIXED_CODES; the mixed point has one path.

A vector quantiser of (b, d) vectors is described by
  codebook   float64 (kmax, d)  the codewords; the slots past k are never read
  k          int32   [1]        codewords in use
  lengths    float64 [kmax]     bits per codeword (only read when the Lagrange
                                multiplier is non-zero)
Every function that takes `codebook` accepts the dictionary vector_lloyd
returns, the pair (codebook, k), or a (k, d) array alone; numpy arrays are
uploaded, device tensors are used as they are.

Argument convention.  The reference's arrays are (s, b), one column per
sample; this package's are (b, s), one row per sample, as everywhere else in
utils.quantization.

Where torch does arithmetic here: the two stated exceptions of
utils.quantization, in their vector form -- vector_lloyd forms the initial
lengths -log2(count / n) from integer counts with torch.log2, once per fit,
and gathers its single host read through one float64 torch.cat.  Everything
else torch does is plumbing: column gathers, index_copy_, views.
"""
import ctypes
from collections import namedtuple as _namedtuple

import numpy as np
import torch

import vtc_hip
from utils import index_coding as _coding
from utils import quantization as _scalar
from utils.quantization import *   # noqa: F401,F403  (a superset of it)
from utils.quantization import (   # noqa: F401  the names the experiment uses
    assign, scalar_lloyd, index_counts, dequantize_assignments, entropy_bits,
    uniform_codebooks, cbook_inds_of_zero_pts, compute_RD_point,
    jpeg_compute_RD_point, baseline_compute_RD_point, Mod1_compute_RD_point)

VQ_MAX_DIM = vtc_hip.VQ_MAX_DIM
VQ_MAX_CODEWORDS = vtc_hip.VQ_MAX_CODEWORDS
VQ_LARGE_MAX_CODEWORDS = vtc_hip.VQ_LARGE_MAX_CODEWORDS


def _limit(max_codewords):
  max_codewords = int(max_codewords)
  if not 1 <= max_codewords <= VQ_LARGE_MAX_CODEWORDS:
    raise ValueError('max_codewords = %d, from 1 to %d'
                     % (max_codewords, VQ_LARGE_MAX_CODEWORDS))
  return max_codewords


def _entry(lib, name, kmax):
  """The entry point `name` for a codebook of kmax slots: include/vtc_vq.h up
  to 4096 of them, include/vtc_vq_large.h above."""
  prefix = 'vtc_vq_' if kmax <= VQ_MAX_CODEWORDS else 'vtc_vq_large_'
  return getattr(lib, prefix + name), prefix + name


# ------------------------------------------------------------------ host side
def _initial_codebook_host(vectors, num_bins, max_codewords=VQ_MAX_CODEWORDS):
  """initial_vector_codebook on a (b, d) numpy array: float64 (k, d)."""
  vectors = np.asarray(vectors, dtype=np.float32)
  b, d = vectors.shape
  max_codewords = _limit(max_codewords)
  m = max(1, min(int(num_bins), b, max_codewords))
  picked = vectors[(np.arange(m, dtype=np.int64) * b) // m]
  picked = picked[~np.isnan(picked).any(1)]
  rows = np.concatenate([np.zeros((1, d), np.float32), picked])
  rows = np.where(rows == 0, np.float32(0.0), rows)          # -0.0 is 0.0
  keys = np.ascontiguousarray(rows).view(np.uint32).reshape(len(rows), d)
  _, first = np.unique(keys, axis=0, return_index=True)
  return rows[np.sort(first)][:max_codewords].astype(np.float64)


def _vectors(vectors, name='vectors'):
  vectors = vtc_hip.require_device_tensor(vectors, name)
  if vectors.dim() != 2 or vectors.numel() == 0:
    raise ValueError('%s must be (b, d), got shape %s'
                     % (name, tuple(vectors.shape)))
  if vectors.shape[1] > VQ_MAX_DIM:
    raise NotImplementedError('d = %d, at most %d'
                              % (vectors.shape[1], VQ_MAX_DIM))
  return vectors.contiguous()


def _device_codebook(codebook, d, device, max_codewords=VQ_MAX_CODEWORDS):
  """(codebook float64 (kmax, d), k int32 [1], lengths or None) on `device`."""
  max_codewords = _limit(max_codewords)
  lengths, k = None, None
  if isinstance(codebook, dict):
    lengths = codebook.get('lengths')
    codebook, k = codebook['codebook'], codebook['k']
  elif isinstance(codebook, (tuple, list)) and len(codebook) == 2:
    codebook, k = codebook
  if len(codebook.shape) != 2 or codebook.shape[1] != d:
    raise ValueError('codebook must be (kmax, %d), got shape %s'
                     % (d, tuple(codebook.shape)))
  kmax = int(codebook.shape[0])
  if kmax < 1:
    raise ValueError('codebook must hold at least one codeword')
  if kmax > max(max_codewords, VQ_MAX_CODEWORDS):
    raise NotImplementedError('kmax = %d, at most %d'
                              % (kmax, max(max_codewords, VQ_MAX_CODEWORDS)))
  if k is None:
    k = np.array([kmax], np.int32)
  elif not torch.is_tensor(k):
    k = np.asarray(k, dtype=np.int32).reshape(1)
  return (_scalar._on(device, codebook, torch.float64, (kmax, d), 'codebook'),
          _scalar._on(device, k, torch.int32, (1,), 'k'), lengths)


# ---------------------------------------------------------------- device side
def initial_vector_codebook(vectors, num_bins, max_codewords=VQ_MAX_CODEWORDS):
  """A deterministic starting codebook for vector_lloyd: float64 (k, d) device
  tensor whose row 0 is the zero vector.

  The candidates are the rows floor(i * b / m), i = 0 .. m - 1, of the (b, d)
  float32 device tensor `vectors`, with m = min(num_bins, b, max_codewords);
  rows with a NaN are skipped, the zero vector is put in front, bitwise
  duplicates are removed (first occurrences stay, -0.0 counts as 0.0) and at
  most max_codewords rows are kept.  Plumbing: a gather on the device, one
  transfer, the comparison of at most max_codewords + 1 rows on the host.

  max_codewords is 4096 unless the caller raises it (at most 131072): the
  experiment passes vec_init_num_bins = 100000, and with
  max_codewords = 131072 that call starts the fit from every distinct
  candidate (module docstring)."""
  vectors = _vectors(vectors)
  b = vectors.shape[0]
  max_codewords = _limit(max_codewords)
  m = max(1, min(int(num_bins), b, max_codewords))
  # the same rows as _initial_codebook_host picks: floor(i * b / m) of m rows
  rows = (torch.arange(m, dtype=torch.int64, device=vectors.device) * b) // m
  picked = vectors.index_select(0, rows).cpu().numpy()
  return torch.from_numpy(
      _initial_codebook_host(picked, m, max_codewords)).to(vectors.device)


def vector_assign(vectors, codebook, lengths=None, lagrange_mult=0.0,
                  return_dequantized=False, max_codewords=VQ_MAX_CODEWORDS):
  """indices [b] int32: for every row of the (b, d) float32 device tensor the
  lowest index i < k that minimises |x - c_i|^2 + lagrange_mult * lengths[i]
  in float64, the squared distance accumulated component by component
  (include/vtc_vq.h); with lagrange_mult == 0 the nearest codeword, lengths
  unused.  Ties go to the lowest index; a row with a NaN gets -1.  With
  return_dequantized also the (b, d) float32 codewords.  A codebook of more
  than 4096 slots needs max_codewords (module docstring).  Only enqueues."""
  out = _vector_assign(vectors, codebook, lengths, lagrange_mult,
                       return_dequantized, max_codewords)
  return (out[0], out[1]) if return_dequantized else out[0]


def _vector_assign(vectors, codebook, lengths, lagrange_mult,
                   return_dequantized, max_codewords=VQ_MAX_CODEWORDS):
  lib = vtc_hip.load_library()
  vectors = _vectors(vectors)
  b, d = vectors.shape
  device = vectors.device
  values, k, own_lengths = _device_codebook(codebook, d, device, max_codewords)
  kmax = values.shape[0]
  if lengths is None:
    lengths = own_lengths
  if lagrange_mult != 0 and lengths is None:
    raise ValueError('a non-zero lagrange_mult needs the codeword lengths')
  if lagrange_mult == 0:
    lengths = None
  if lengths is not None:
    lengths = _scalar._on(device, lengths, torch.float64, (kmax,), 'lengths')
  indices = torch.empty(b, dtype=torch.int32, device=device)
  dequantized = (torch.empty((b, d), dtype=torch.float32, device=device)
                 if return_dequantized else None)
  status = torch.empty(1, dtype=torch.int64, device=device)
  assign_entry, name = _entry(lib, 'assign', kmax)
  vtc_hip.check(assign_entry(
      vtc_hip.ptr(vectors), b, d, vtc_hip.ptr(values), vtc_hip.ptr(lengths),
      vtc_hip.ptr(k), kmax, float(lagrange_mult), vtc_hip.ptr(indices),
      vtc_hip.ptr(dequantized), vtc_hip.ptr(status),
      vtc_hip.current_stream(device)), name)
  return indices, dequantized, status


def vector_index_counts(indices, kmax, max_codewords=VQ_MAX_CODEWORDS):
  """int64 [kmax] device tensor: how often each index 0 .. kmax - 1 occurs in
  the [b] int32 device tensor `indices`; the -1 of a NaN row is not counted.
  kmax > 4096 needs max_codewords (module docstring).  Only enqueues."""
  lib = vtc_hip.load_library()
  indices = vtc_hip.require_device_tensor(indices, 'indices', torch.int32)
  if indices.dim() != 1 or indices.numel() == 0:
    raise ValueError('indices must be [b], got shape %s'
                     % (tuple(indices.shape),))
  indices = indices.contiguous()
  kmax = int(kmax)
  limit = max(_limit(max_codewords), VQ_MAX_CODEWORDS)
  if kmax > limit:
    raise NotImplementedError('kmax = %d, at most %d' % (kmax, limit))
  counts = torch.empty(max(kmax, 1), dtype=torch.int64, device=indices.device)
  counts_entry, name = _entry(lib, 'index_counts', kmax)
  vtc_hip.check(counts_entry(
      vtc_hip.ptr(indices), indices.shape[0], kmax, vtc_hip.ptr(counts),
      vtc_hip.current_stream(indices.device)), name)
  return counts


def vector_dequantize(indices, codebook, max_codewords=VQ_MAX_CODEWORDS):
  """(b, d) float32 device tensor of codebook[indices[r]] rounded once to
  float32, a row of NaN where the index is -1.  A gather: tensor plumbing done
  by torch on the tensor's device.  A codebook of more than 4096 slots needs
  max_codewords (module docstring).  Only enqueues."""
  indices = vtc_hip.require_device_tensor(indices, 'indices', torch.int32)
  if indices.dim() != 1:
    raise ValueError('indices must be [b], got shape %s'
                     % (tuple(indices.shape),))
  if isinstance(codebook, dict):
    codebook = codebook['codebook']
  elif isinstance(codebook, (tuple, list)) and len(codebook) == 2:
    codebook = codebook[0]
  values, _, _ = _device_codebook(codebook, codebook.shape[1], indices.device,
                                  max_codewords)
  picked = values.index_select(0, indices.clamp(min=0).to(torch.int64))
  picked = picked.to(torch.float32)
  return torch.where((indices < 0)[:, None],
                     torch.full_like(picked, float('nan')), picked)


def _state(tensors):
  return vtc_hip.VqState(**{name: t.data_ptr()
                            for name, t in tensors.items()})


def vector_lloyd(vectors, init_codebook, lagrange_mult=0.0, max_iterations=50,
                 epsilon=1e-5, pin_zero=True, max_codewords=VQ_MAX_CODEWORDS):
  """An entropy-constrained vector quantiser for the rows of the (b, d)
  float32 device tensor `vectors`, fitted on the device: the twin of
  scalar_lloyd.

  The fit starts from init_codebook ((k, d), e.g. initial_vector_codebook)
  with the lengths -log2(count / n) of the nearest-codeword assignment, then
  takes up to max_iterations steps of vtc_vq_lloyd_step: assign under
  |x - c|^2 + lagrange_mult * length, move every codeword to the mean of its
  members, drop the codewords without members, set length = -log2(count / n).
  The fit stops when its cost J = D + lagrange_mult * R improves by no more
  than epsilon * J; that test is made on the device, and the max_iterations
  steps are enqueued without a host read between them.  With pin_zero the
  codeword that is exactly the zero vector stays there and is never dropped.

  Returns a dictionary: 'codebook' float64 (kmax, d), 'lengths' float64
  [kmax], 'counts' int64 [kmax], 'k' int32 [1], 'zero_index' int32 [1] as
  device tensors (slots past k: 0.0, 0.0, 0), and, read once at the end,
  'iterations' (int), 'converged' (bool) and 'cost' float64 [3] = {J, D, R}
  of the last step (numpy).  A NaN in the vectors raises ValueError.

  An init_codebook of more than 4096 rows needs max_codewords (module
  docstring); the fit keeps its kmax slots however few stay in use, and
  trim_vector_codebook cuts the result down to them.
  """
  lib = vtc_hip.load_library()
  vectors = _vectors(vectors)
  b, d = vectors.shape
  device = vectors.device
  if isinstance(init_codebook, dict):
    init_codebook = (init_codebook['codebook'], init_codebook['k'])
  values, k, _ = _device_codebook(init_codebook, d, device, max_codewords)
  values, k = values.clone(), k.clone()      # the fit is in place
  kmax = values.shape[0]
  # the zero codeword of the start: plumbing (comparisons) on the device
  in_use = torch.arange(kmax, device=device) < k.to(torch.int64)
  is_zero = (values == 0).all(1) & in_use
  zero = torch.where(is_zero.any(), is_zero.to(torch.int32).argmax(),
                     torch.tensor(-1, device=device)).to(torch.int32)
  indices, _, first_status = _vector_assign(vectors, (values, k), None, 0.0,
                                            False, max_codewords)
  counts = vector_index_counts(indices, kmax, max_codewords)
  del indices
  # the first step's input lengths, by torch (module docstring)
  lengths = -torch.log2(counts.to(torch.float64) /
                        counts.sum().to(torch.float64))
  tensors = {
      'codebook': values, 'lengths': lengths.contiguous(), 'counts': counts,
      'cost': torch.zeros(3, dtype=torch.float64, device=device),
      'k': k, 'zero_index': zero.reshape(1).contiguous(),
      'active': torch.ones(1, dtype=torch.int32, device=device),
      'iterations': torch.zeros(1, dtype=torch.int32, device=device)}
  state = _state(tensors)
  status = torch.zeros(1, dtype=torch.int64, device=device)
  step_bytes, _ = _entry(lib, 'lloyd_step_workspace_bytes', kmax)
  step_entry, step_name = _entry(lib, 'lloyd_step', kmax)
  ws = vtc_hip.workspace(step_bytes(b, d, kmax), device)
  stream = vtc_hip.current_stream(device)
  for _ in range(int(max_iterations)):
    vtc_hip.check(step_entry(
        vtc_hip.ptr(vectors), b, d, kmax, float(lagrange_mult),
        float(epsilon), 1 if pin_zero else 0, ctypes.byref(state),
        ctypes.byref(state), vtc_hip.ptr(status), vtc_hip.ptr(ws), ws.numel(),
        stream), step_name)
  # the one read: everything as float64 in one buffer (module docstring)
  tail = torch.cat([tensors['active'].to(torch.float64),
                    tensors['iterations'].to(torch.float64),
                    tensors['cost'],
                    (status + first_status).to(torch.float64)]).cpu().numpy()
  if tail[-1] != 0:
    raise ValueError('vector_lloyd: the vectors hold NaN')
  result = {name: tensors[name] for name in
            ('codebook', 'k', 'lengths', 'counts', 'zero_index')}
  result['iterations'] = int(tail[1])
  result['converged'] = bool(tail[0] == 0)
  result['cost'] = tail[2:5].copy()
  return result


def trim_vector_codebook(result):
  """The quantiser of vector_lloyd's dictionary `result` with kmax = k: the
  slots in use of 'codebook', 'lengths' and 'counts' (copies), every other
  entry as it is.  It assigns exactly as `result` does, since the slots past k
  are never read.  A fit that started above 4096 codewords and ended at or
  below them is thereby handed to everything that takes at most 4096, the
  Huffman and range coders of the indices included.  One host read (k)."""
  k = int(result['k'].reshape(-1)[0])
  trimmed = dict(result)
  for name in ('codebook', 'lengths', 'counts'):
    trimmed[name] = result[name][:k].clone()
  trimmed['k'] = result['k'].clone()
  return trimmed


def _slots(codebook):
  """kmax of a codebook in any of the accepted forms, without touching it."""
  if isinstance(codebook, dict):
    codebook = codebook['codebook']
  elif isinstance(codebook, (tuple, list)) and len(codebook) == 2:
    codebook = codebook[0]
  return int(codebook.shape[0])


# ------------------------------------------------------------- rate-distortion
def _cluster(cluster, s, name):
  cluster = [int(c) for c in cluster]
  if not cluster:
    raise ValueError('%s is empty' % name)
  if min(cluster) < 0 or max(cluster) >= s:
    raise ValueError('%s falls outside [0, %d)' % (name, s))
  return cluster


def _clusters(scal_clusts, vec_clust, s):
  """The scalar and the vector columns as lists of ints: inside [0, s), not
  overlapping."""
  scal = _cluster(scal_clusts, s, 'scal_clusts')
  vec = _cluster(vec_clust, s, 'vec_clust')
  if len(set(scal + vec)) != len(scal) + len(vec):
    raise ValueError('scal_clusts and vec_clust overlap')
  return scal, vec


def _scatter(s, *parts):
  """The (b, s) float32 codes that hold every part = (columns, dequantised
  values (b, len(columns))), a coefficient in no part zero."""
  values = parts[0][1]
  codes = torch.zeros((values.shape[0], s), dtype=torch.float32,
                      device=values.device)
  for columns, values in parts:
    codes.index_copy_(1, torch.as_tensor(columns, dtype=torch.int64,
                                         device=codes.device), values)
  return codes


def _stacked_frequencies(scalar_freq, vector_freq):
  """The uint16 (len(scal_clusts) + 1, kmax) frequencies of the combined index
  array: the scalar rows, then the vector row, padded with zeros (absent
  symbols) to the larger kmax."""
  scalar_freq = np.asarray(scalar_freq)
  vector_freq = np.asarray(vector_freq).reshape(1, -1)
  if scalar_freq.ndim != 2:
    raise ValueError('the scalar frequencies must be (len(scal_clusts), kmax)')
  kmax = max(scalar_freq.shape[1], vector_freq.shape[1])
  out = np.zeros((scalar_freq.shape[0] + 1, kmax), dtype=np.uint16)
  out[:-1, :scalar_freq.shape[1]] = scalar_freq
  out[-1, :vector_freq.shape[1]] = vector_freq[0]
  return out


# What a mixed point codes under each source code: the coder of the scalar
# columns, the coder of the vector column and, where both go into ONE stream
# set over the (b, len(scal_clusts) + 1) array [scalar columns ..., vector
# column], how the pair `tables` = (scalar tables, vector table) is joined for
# it.  join None: a stream set each (under 'entropy': none).
_MixedCode = _namedtuple('_MixedCode', 'scalar vector join')
_MIXED_CODES = {
    'entropy': _MixedCode(_coding.Entropy, _coding.Entropy, None),
    'huffman': _MixedCode(_coding.Huffman, _coding.Huffman,
                          lambda scalar, vector: list(scalar) + [vector]),
    'ans': _MixedCode(_coding.Ans, _coding.Ans,
                      _stacked_frequencies),
    'ans_split': _MixedCode(_coding.Ans, _coding.AnsSplit, None)}


def compute_RD_point_mixed(codes, patches, dictionary, scal_clusts,
                           scal_codebooks, vec_clust, vec_codebook,
                           scal_lengths=None, scal_lagrange_mult=0.0,
                           vec_lengths=None, vec_lagrange_mult=0.0,
                           fullimg_reshape_params=None, source_code='entropy',
                           tables=None, from_stream=False,
                           rows_per_stream=None,
                           vec_max_codewords=VQ_MAX_CODEWORDS):
  """One rate-distortion point of codes quantised in two parts.

  codes : (b, s) float32 device tensor; patches : (b, n); dictionary : (s, n),
  patches ~ codes @ dictionary.  The columns scal_clusts (a list of column
  numbers) go through quantization.assign with one scalar quantiser each
  (scal_codebooks, scal_lengths, scal_lagrange_mult: row j of the codebooks
  belongs to column scal_clusts[j]); the columns vec_clust are quantised as
  one vector per row by vector_assign (vec_codebook, vec_lengths,
  vec_lagrange_mult).  A coefficient in neither cluster is set to zero and
  costs no bits.  Overlapping clusters, or clusters that fall outside [0, s),
  raise ValueError.

  Returns (rate, distortion): the rate is (the sum over the scalar columns of
  the empirical entropy of their indices + the entropy of the vector indices)
  / patches.numel() in bits per pixel (entropy_bits); reconstruction and
  distortion are those of compute_RD_point.

  source_code 'huffman': the scalar indices and the vector index form one
  (b, len(scal_clusts) + 1) index array, scalars first in scal_clusts order,
  the vector column last, and every column is coded under a Huffman table of
  its own (utils.index_coding; the tables are padded to the larger kmax).
  `tables` = (scalar_tables, vector_table): a list of len(scal_clusts) dicts
  and one dict, trained on these indices when None.  The rate is the total of
  index_code_bits / patches.numel(), and a third value is returned: the
  tables.

  source_code 'ans': the same index array under the range coder of
  quantization.compute_RD_point.  `tables` = (scalar frequencies uint16
  (len(scal_clusts), kmax), vector frequencies uint16 (kmax',)), trained on
  these indices when None and padded with zeros to the larger kmax for the
  device; the rate is 8 x the bytes of the streams of rows_per_stream rows /
  patches.numel(), and the third value is that pair.

  from_stream (source_code 'huffman' and 'ans' only, ValueError otherwise):
  that index array is packed with index_coding.pack_index_streams
  (pack_index_ans) and read back by decode_codes_mixed; reconstruction and
  distortion are those of the decoded codes and the rate is the streams' total
  bits / patches.numel().

  source_code 'ans_split': the scalar indices (b, len(scal_clusts)) go through
  the range coder as under 'ans', and the vector index through the split range
  coder of include/ext/vtc_index_ans_split.h (index_coding.pack_index_ans_split)
  as a stream set of its own, which takes up to 131072 symbols.  `tables` =
  (scalar frequencies uint16 (len(scal_clusts), kmax), (freq_hi, freq_lo)),
  trained on these indices when None (index_ans_frequencies,
  index_ans_split_frequencies) and returned as the third value.  The rate is
  8 x the bytes of both stream sets / patches.numel(); rows_per_stream applies
  to both, and None means each coder's default.  from_stream decodes both with
  decode_codes_mixed_split.

  vec_max_codewords: a vec_codebook of more than 4096 slots needs it (module
  docstring), and then source_code must be 'entropy' or 'ans_split': 'huffman'
  and 'ans' raise NotImplementedError before any device work."""
  _scalar._source_coder(source_code, from_stream, mixed=True)
  code = _MIXED_CODES[source_code]
  limit = code.vector.max_symbols
  # a coder with a symbol for every index of the largest quantiser is not
  # asked: a codebook beyond that is _device_codebook's to refuse
  if limit < VQ_LARGE_MAX_CODEWORDS and _slots(vec_codebook) > limit:
    raise NotImplementedError(
        "source_code %r codes at most %d symbols and the vector codebook has "
        "kmax = %d slots: cut a fit that ended at k <= %d down with "
        "trim_vector_codebook" % (source_code, limit, _slots(vec_codebook),
                                  limit))
  codes = _scalar._codes(codes)
  patches = _scalar._codes(patches, 'patches')
  if patches.shape[0] != codes.shape[0]:
    raise ValueError('one patch per row of codes')
  b, s = codes.shape
  device = codes.device
  scal, vec = _clusters(scal_clusts, vec_clust, s)
  scal_at = torch.tensor(scal, dtype=torch.int64, device=device)
  vec_at = torch.tensor(vec, dtype=torch.int64, device=device)

  scal_pair = _scalar._device_pair(scal_codebooks, len(scal), device)
  if scal_lengths is None and isinstance(scal_codebooks, dict):
    scal_lengths = scal_codebooks.get('lengths')
  scal_indices, scal_deq, scal_status = _scalar._assign(
      codes.index_select(1, scal_at).contiguous(), scal_pair, scal_lengths,
      scal_lagrange_mult, True)
  vec_values, vec_k, own_lengths = _device_codebook(vec_codebook, len(vec),
                                                    device, vec_max_codewords)
  if vec_lengths is None:
    vec_lengths = own_lengths
  vec_indices, vec_deq, vec_status = _vector_assign(
      codes.index_select(1, vec_at).contiguous(), (vec_values, vec_k),
      vec_lengths, vec_lagrange_mult, True, vec_max_codewords)

  dequantized = _scatter(s, (scal_at, scal_deq), (vec_at, vec_deq))
  if not from_stream:
    reconstruction = _scalar._reconstruct(dequantized, dictionary)
  if int(scal_status) != 0 or int(vec_status) != 0:
    raise ValueError('compute_RD_point_mixed: the codes hold NaN')
  scal_counts = lambda: index_counts(scal_indices, scal_pair[0].shape[1])
  vec_counts = lambda: vector_index_counts(vec_indices, vec_values.shape[0],
                                           vec_max_codewords)
  if not code.scalar.has_tables:
    total_bits = (entropy_bits(scal_counts()) +
                  entropy_bits(vec_counts()[None, :]))
  else:
    if tables is None:
      tables = (code.scalar.train(scal_counts(), scal_pair[1]),
                code.vector.train_column(vec_counts(), vec_k))
    # what is coded, as (coder, indices, tables): the scalar and the vector
    # part, or one part over the joined index array
    parts = [(code.scalar, scal_indices, tables[0]),
             (code.vector, vec_indices, tables[1])]
    if code.join is not None:
      parts = [(code.scalar, torch.cat([scal_indices, vec_indices[:, None]], 1),
                code.join(*tables))]
    if from_stream:
      parts = [(coder, coder.pack(indices, part_tables, rows_per_stream),
                part_tables) for coder, indices, part_tables in parts]
      total_bits = sum(streams.bits for _, streams, _ in parts)
      reconstruction = _scalar._reconstruct(
          _decode_mixed(parts, scal_at, scal_pair, vec_at,
                        (vec_values, vec_k), s, vec_max_codewords), dictionary)
    else:
      total_bits = sum(
          coder.total_bits(indices, part_tables, rows_per_stream)
          for coder, indices, part_tables in parts)
  rate = total_bits / float(patches.numel())
  distortion = _scalar._distortion(patches, reconstruction,
                                   fullimg_reshape_params)
  if code.scalar.has_tables:
    return rate, distortion, tuple(tables)
  return rate, distortion


def _decode_mixed(parts, scal, scal_codebooks, vec, vec_codebook, s,
                  vec_max_codewords=VQ_MAX_CODEWORDS):
  """The (b, s) dequantised codes of the stream sets in parts = [(coder,
  stream set, tables)], one part for the joined index array or the scalar and
  the vector part: unpack, quantization.dequantize_assignments into the
  columns `scal`, vector_dequantize into the columns `vec`."""
  indices = [coder.unpack(streams, tables) for coder, streams, tables in parts]
  if len(indices) == 1:
    scal_indices = indices[0][:, :len(scal)].contiguous()
    vec_indices = indices[0][:, len(scal)].contiguous()
  else:
    scal_indices, vec_indices = indices
  scal_deq = _scalar.dequantize_assignments(scal_indices, scal_codebooks)
  vec_deq = vector_dequantize(vec_indices, vec_codebook, vec_max_codewords)
  if vec_deq.shape[1] != len(vec):
    raise ValueError('vec_codebook must be (kmax, %d)' % len(vec))
  return _scatter(s, (scal, scal_deq), (vec, vec_deq))


def decode_codes_mixed(packed, offsets, tables, scal_clusts, scal_codebooks,
                       vec_clust, vec_codebook, s, ans_shape=None):
  """The (b, s) float32 dequantised codes whose index streams are in (packed,
  offsets), the layout compute_RD_point_mixed codes: one row per patch, the
  scalar indices first in scal_clusts order, the vector index last.  `tables`
  is the list of len(scal_clusts) + 1 tables in that order.
  index_coding.unpack_index_streams, then quantization.dequantize_assignments
  into the columns scal_clusts and vector_dequantize into the columns
  vec_clust; a column in neither cluster is zero.  One host read (the
  decoder's status).

  ans_shape = (b, rows_per_stream): the streams are those of
  index_coding.pack_index_ans, `tables` the uint16 (len(scal_clusts) + 1,
  kmax) frequencies in that order, read by index_coding.unpack_index_ans."""
  s = int(s)
  scal, vec = _clusters(scal_clusts, vec_clust, s)
  coder, streams = _scalar._stream_set(packed, offsets, ans_shape)
  if coder is _coding.Huffman:
    tables = list(tables)
  if len(tables) != len(scal) + 1:
    raise ValueError('%d tables for %d scalar columns and the vector column'
                     % (len(tables), len(scal)))
  return _decode_mixed([(coder, streams, tables)], scal, scal_codebooks, vec,
                       vec_codebook, s)


def decode_codes_mixed_split(scalar_streams, vector_streams, tables,
                             scal_clusts, scal_codebooks, vec_clust,
                             vec_codebook, s, b,
                             vec_max_codewords=VQ_MAX_CODEWORDS):
  """The (b, s) float32 dequantised codes of the two stream sets that
  compute_RD_point_mixed writes under source_code='ans_split':
  scalar_streams = (packed, offsets, rows_per_stream) of
  index_coding.pack_index_ans for the (b, len(scal_clusts)) scalar indices,
  vector_streams the same of index_coding.pack_index_ans_split for the [b]
  vector indices, tables = (scalar frequencies, (freq_hi, freq_lo)).  Then
  quantization.dequantize_assignments into the columns scal_clusts and
  vector_dequantize (with vec_max_codewords) into the columns vec_clust; a
  column in neither cluster is zero.  Two host reads (the decoders'
  statuses)."""
  s, b = int(s), int(b)
  scal, vec = _clusters(scal_clusts, vec_clust, s)
  scalar_tables, vector_table = tables
  if len(scalar_tables) != len(scal):
    raise ValueError('%d rows of frequencies for %d scalar columns'
                     % (len(scalar_tables), len(scal)))
  code = _MIXED_CODES['ans_split']
  stream_set = lambda streams: _coding.StreamSet(streams[0], streams[1], b,
                                                 streams[2], None)
  return _decode_mixed(
      [(code.scalar, stream_set(scalar_streams), scalar_tables),
       (code.vector, stream_set(vector_streams), vector_table)],
      scal, scal_codebooks, vec, vec_codebook, s, vec_max_codewords)


def _gathered(codes, cluster):
  codes = _scalar._codes(codes)
  cluster = _cluster(cluster, codes.shape[1], 'cluster')
  at = torch.tensor(cluster, dtype=torch.int64, device=codes.device)
  return codes.index_select(1, at).contiguous()


def _fit_vector_part(codes, vec_clust, vec_quant_multiplier, vec_init_num_bins,
                     max_iterations, epsilon, source_code, max_codewords):
  """(the dictionary of vector_lloyd, its 'lengths').  A fit of more than 4096
  slots that a table code is to follow is cut down to its slots in use."""
  vectors = _gathered(codes, vec_clust)
  fitted = vector_lloyd(
      vectors,
      initial_vector_codebook(vectors, vec_init_num_bins, max_codewords),
      lagrange_mult=vec_quant_multiplier, max_iterations=max_iterations,
      epsilon=epsilon, max_codewords=max_codewords)
  code = _MIXED_CODES.get(source_code)   # _mixed_point refuses other names
  if code and _slots(fitted) > code.vector.max_symbols:
    fitted = trim_vector_codebook(fitted)
  return fitted, fitted['lengths']


def _mixed_point(who, training, source_code, from_stream, rows_per_stream,
                 huff_tab1, huff_tab2, *args, **kwargs):
  """compute_RD_point_mixed for Mod2 / Mod3: (rate, distortion, huff_tab1,
  huff_tab2), the two tables None under 'entropy'."""
  coder = _scalar._source_coder(source_code, from_stream, mixed=True)
  if not coder.has_tables:
    return compute_RD_point_mixed(*args, **kwargs) + (None, None)
  tables = None
  if not training:
    _scalar._need_tables(who, coder, huff_tab1, huff_tab2)
    tables = (huff_tab1, huff_tab2)
  rate, distortion, tables = compute_RD_point_mixed(
      *args, source_code=source_code, tables=tables, from_stream=from_stream,
      rows_per_stream=rows_per_stream, **kwargs)
  return rate, distortion, tables[0], tables[1]


def Mod2_compute_RD_point(codes, patches, dictionary, scal_clusts, vec_clust,
                          scal_quant_multiplier=1.0, scal_binwidths=None,
                          vec_quant_multiplier=1.0, vec_init_num_bins=4096,
                          precomputed_scal_codebook=None,
                          precomputed_vec_codebook=None,
                          precomputed_vec_codebook_lengths=None,
                          precomputed_huff_tab1=None,
                          precomputed_huff_tab2=None,
                          precomputed_huff_tab3=None,
                          fullimg_reshape_params=None, max_iterations=50,
                          epsilon=1e-5, source_code='entropy',
                          from_stream=False, rows_per_stream=None,
                          vec_max_codewords=VQ_MAX_CODEWORDS):
  """The experiment's Mod2_compute_RD_point, with (b, s) codes (module
  docstring): the columns scal_clusts get uniform scalar codebooks of bin
  width scal_binwidths * scal_quant_multiplier (as in
  baseline_compute_RD_point), the columns vec_clust one entropy-constrained
  vector quantiser, vector_lloyd from initial_vector_codebook(.,
  vec_init_num_bins) with lagrange_mult = vec_quant_multiplier; every index
  stream is coded at its empirical entropy (compute_RD_point_mixed).

  Training call (no precomputed_*): returns the experiment's 8-tuple (rate,
  distortion, scal_cbook, vec_cbook, vec_cw_len, None, None, None): the pair
  of uniform_codebooks, the dictionary of vector_lloyd and its 'lengths'; the
  three Huffman table slots are None for the reason
  baseline_compute_RD_point's docstring gives (and the precomputed_huff_tab*
  arguments are accepted and unused).  Test call (precomputed_scal_codebook,
  precomputed_vec_codebook, precomputed_vec_codebook_lengths): returns
  (rate, distortion).

  With source_code='huffman' every index stream is coded under a Huffman
  table of its own instead (compute_RD_point_mixed).  The experiment's missing
  module never said what its three table slots held; here the training call
  returns huff_tab1 = the list of len(scal_clusts) scalar tables, huff_tab2 =
  the vector table, huff_tab3 = None, and a test call takes the first two back
  as precomputed_huff_tab1 and precomputed_huff_tab2 and measures the bits of
  the test indices under them.  Precomputed codebooks without both tables
  raise ValueError.  from_stream is that of compute_RD_point_mixed, and so
  are source_code='ans' and rows_per_stream: huff_tab1 and huff_tab2 are then
  the scalar and the vector frequency arrays.

  vec_max_codewords (4096, at most 131072) goes to initial_vector_codebook,
  vector_lloyd and compute_RD_point_mixed: with vec_max_codewords=131072 the
  experiment's vec_init_num_bins=100000 starts the fit from every distinct
  candidate.  The returned vec_cbook keeps the slots it started with;
  source_code 'huffman' and 'ans' code at most 4096 symbols, so a training
  call under them cuts a larger fit down with trim_vector_codebook first and
  raises NotImplementedError only if more than 4096 codewords are still in
  use.  source_code='ans_split' (compute_RD_point_mixed) codes the vector
  index with up to 131072 symbols: nothing is cut down, huff_tab1 is the
  scalar frequency array and huff_tab2 the pair (freq_hi, freq_lo)."""
  training = precomputed_scal_codebook is None
  if training:
    scal_cbook = _scalar._uniform_for(_gathered(codes, scal_clusts),
                                      scal_binwidths, scal_quant_multiplier)
    vec_cbook, vec_cw_len = _fit_vector_part(
        codes, vec_clust, vec_quant_multiplier, vec_init_num_bins,
        max_iterations, epsilon, source_code, vec_max_codewords)
  else:
    scal_cbook, vec_cbook, vec_cw_len = (precomputed_scal_codebook,
                                         precomputed_vec_codebook,
                                         precomputed_vec_codebook_lengths)
  rate, distortion, huff_tab1, huff_tab2 = _mixed_point(
      'Mod2_compute_RD_point', training, source_code, from_stream,
      rows_per_stream,
      precomputed_huff_tab1, precomputed_huff_tab2,
      codes, patches, dictionary, scal_clusts, scal_cbook, vec_clust,
      vec_cbook, vec_lengths=vec_cw_len,
      vec_lagrange_mult=vec_quant_multiplier,
      fullimg_reshape_params=fullimg_reshape_params,
      vec_max_codewords=vec_max_codewords)
  if training:
    return (rate, distortion, scal_cbook, vec_cbook, vec_cw_len, huff_tab1,
            huff_tab2, None)
  return rate, distortion


def Mod3_compute_RD_point(codes, patches, dictionary, scal_clusts, vec_clust,
                          scal_quant_multiplier=1.0, scal_binwidths=None,
                          vec_quant_multiplier=1.0, vec_init_num_bins=4096,
                          precomputed_scal_codebook=None,
                          precomputed_vec_codebook=None,
                          precomputed_vec_codebook_lengths=None,
                          precomputed_huff_tab1=None,
                          precomputed_huff_tab2=None,
                          precomputed_huff_tab3=None,
                          fullimg_reshape_params=None, max_iterations=50,
                          epsilon=1e-5, source_code='entropy',
                          from_stream=False, rows_per_stream=None,
                          vec_max_codewords=VQ_MAX_CODEWORDS):
  """The experiment's Mod3_compute_RD_point: Mod2_compute_RD_point with
  entropy-constrained scalar quantisers, scalar_lloyd from uniform codebooks
  of bin width scal_binwidths with lagrange_mult = scal_quant_multiplier (as
  in Mod1_compute_RD_point).  The experiment's test call does not pass the
  scalar multiplier again, so the returned scal_cbook is scalar_lloyd's
  dictionary with one more key, 'lagrange_mult', and a test call assigns with
  that value and the dictionary's 'lengths'.  Returns as Mod2_compute_RD_point
  does, source_code='huffman' and 'ans', their table slots, from_stream,
  rows_per_stream and vec_max_codewords included."""
  training = precomputed_scal_codebook is None
  if training:
    scal_codes = _gathered(codes, scal_clusts)
    scal_cbook = scalar_lloyd(
        scal_codes, _scalar._uniform_for(scal_codes, scal_binwidths, 1.0),
        lagrange_mult=scal_quant_multiplier, max_iterations=max_iterations,
        epsilon=epsilon)
    scal_cbook['lagrange_mult'] = scal_quant_multiplier
    vec_cbook, vec_cw_len = _fit_vector_part(
        codes, vec_clust, vec_quant_multiplier, vec_init_num_bins,
        max_iterations, epsilon, source_code, vec_max_codewords)
  else:
    scal_cbook, vec_cbook, vec_cw_len = (precomputed_scal_codebook,
                                         precomputed_vec_codebook,
                                         precomputed_vec_codebook_lengths)
  rate, distortion, huff_tab1, huff_tab2 = _mixed_point(
      'Mod3_compute_RD_point', training, source_code, from_stream,
      rows_per_stream,
      precomputed_huff_tab1, precomputed_huff_tab2,
      codes, patches, dictionary, scal_clusts, scal_cbook, vec_clust,
      vec_cbook, scal_lengths=scal_cbook['lengths'],
      scal_lagrange_mult=scal_cbook['lagrange_mult'], vec_lengths=vec_cw_len,
      vec_lagrange_mult=vec_quant_multiplier,
      fullimg_reshape_params=fullimg_reshape_params,
      vec_max_codewords=vec_max_codewords)
  if training:
    return (rate, distortion, scal_cbook, vec_cbook, vec_cw_len, huff_tab1,
            huff_tab2, None)
  return rate, distortion
