"""The host half of the baseline JFIF reader (utils/jfif.py) and the surface
of the sixteenth header, include/ext/vtc_jfif_decode.h: header, binding table
and exports agree; the marker walk on the restatement's files and on foreign
ones; the frame geometry against scan_layout and written out by hand; every
refusal of the walk on byte strings built here.  No GPU needed.

tests/golden/jfif_foreign.npz holds the bytes of five files that PIL 12.2.0
(libjpeg-turbo) wrote of the seeded 96 x 64 image
jfif_decode_data.foreign_image(): Image.save(format='JPEG', quality=85) with
convert('L') and optimize=True ('gray'), subsampling=0, 1, 2 and optimize=True
('444', '422', '420'), and subsampling=2 without optimize, i.e. the Annex K.3
tables with their 16-bit codewords ('420-default-tables');
jfif_decode_data.make_foreign() is the recipe."""
import ctypes
import io
import pathlib
import re

import numpy as np
import pytest

import jfif_data as truth
import jfif_decode_data as dd

REPO = pathlib.Path(__file__).resolve().parent.parent
HEADER = REPO / 'include' / 'ext' / 'vtc_jfif_decode.h'
ENTRY_POINTS = sorted([
    'vtc_jfif_decode_abi_version', 'vtc_jfif_unstuff_bytes_workspace_bytes',
    'vtc_jfif_unstuff_bytes', 'vtc_jfif_unpack_workspace_bytes',
    'vtc_jfif_unpack', 'vtc_jfif_dc_accumulate_workspace_bytes',
    'vtc_jfif_dc_accumulate'])


def _jfif():
  from utils import jfif
  return jfif


def _code(path):
  return re.sub(r'/\*.*?\*/', '', path.read_text(), flags=re.S)


# ------------------------------------------------------ header and bindings
def test_header_bindings_and_exports():
  import vtc_hip
  code = _code(HEADER)
  declared = {m.group(1): m.group(2) for m in re.finditer(
      r'\b(vtc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', code)}
  assert sorted(declared) == ENTRY_POINTS == sorted(
      vtc_hip.JFIF_DECODE_BINDINGS)
  defines = dict(re.findall(r'#define\s+(VTC_[A-Z_]+)\s+(\d+)\b', code))
  assert {k: int(v) for k, v in defines.items()} == {
      'VTC_JFIF_DECODE_ABI_VERSION': vtc_hip.JFIF_DECODE_ABI_VERSION,
      'VTC_JFIF_SUBSEQ_BYTES': vtc_hip.JFIF_SUBSEQ_BYTES,
      'VTC_JFIF_SUBSEQ_PER_GROUP': vtc_hip.JFIF_SUBSEQ_PER_GROUP,
      'VTC_JFIF_DC_TILE': vtc_hip.JFIF_DC_TILE,
      'VTC_JFIF_MAX_SLOTS': vtc_hip.JFIF_MAX_SLOTS}
  assert vtc_hip.JFIF_SUBSEQ_BYTES == dd.SUBSEQ_BYTES == 128
  assert '#include "../vtc_hip.h"' in code and 'asm' not in code
  # disjoint from every other table, and no function of another header named
  for name in dir(vtc_hip):
    if name.endswith(('SIGNATURES', '_BINDINGS')) and (
        name != 'JFIF_DECODE_BINDINGS'):
      assert not set(vtc_hip.JFIF_DECODE_BINDINGS) & set(getattr(vtc_hip,
                                                                 name)), name
  others = sorted((REPO / 'include').glob('*.h')) + [
      p for p in sorted((REPO / 'include' / 'ext').glob('*.h')) if p != HEADER]
  assert len(others) >= 15
  for other in others:
    names = set(re.findall(r'\b(vtc_[a-z0-9_]+)\s*\(', _code(other)))
    assert names and not names & set(
        re.findall(r'\b(vtc_[a-z0-9_]+)\b', code)), other.name
  lib = vtc_hip.load_library()
  raw = ctypes.CDLL(str(vtc_hip.LIBRARY_PATH))
  for name, args in declared.items():
    assert hasattr(raw, name), 'library does not export ' + name
    count = len([a for a in args.split(',') if a.strip() not in ('', 'void')])
    assert len(vtc_hip.JFIF_DECODE_BINDINGS[name][1]) == count, name
    assert getattr(lib, name).argtypes == (
        vtc_hip.JFIF_DECODE_BINDINGS[name][1])
  assert lib.vtc_jfif_decode_abi_version() == 1
  makefile = (REPO / 'vision-transform-codes_amd' / 'csrc' /
              'Makefile').read_text()
  assert 'include/ext/vtc_jfif_decode.h' in makefile
  # the fifteenth header stays where it was
  assert lib.vtc_jfif_abi_version() == vtc_hip.JFIF_ABI_VERSION == 1


def test_bad_arguments_are_answered_before_device_work():
  """Host integers as pointers: nothing is dereferenced."""
  import vtc_hip
  lib = vtc_hip.load_library()
  p = [ctypes.c_void_p((i + 1) << 30) for i in range(12)]
  null = ctypes.c_void_p(0)
  INVALID, WORKSPACE = 1, 3

  def refused(rc, status, *words):
    assert rc == status, (rc, lib.vtc_last_error())
    for word in words:
      assert word in lib.vtc_last_error().decode(), lib.vtc_last_error()

  un = [p[0], 5000, p[1], 5000, p[2], p[3], p[4], 1 << 20, null]
  assert lib.vtc_jfif_unstuff_bytes_workspace_bytes(0) == 0
  assert lib.vtc_jfif_unstuff_bytes_workspace_bytes(-4) == 0
  need = lib.vtc_jfif_unstuff_bytes_workspace_bytes(5000)
  assert need == 3 * 256     # two arrays of three int64, two words
  for i in (0, 2, 4, 5):
    refused(lib.vtc_jfif_unstuff_bytes(*(un[:i] + [null] + un[i + 1:])),
            INVALID, 'vtc_jfif_unstuff_bytes', 'null')
  refused(lib.vtc_jfif_unstuff_bytes(*(un[:1] + [-1] + un[2:])), INVALID,
          'bad size n')
  refused(lib.vtc_jfif_unstuff_bytes(*(un[:3] + [-1] + un[4:])), INVALID,
          'bad size capacity')
  refused(lib.vtc_jfif_unstuff_bytes(*(un[:6] + [null] + un[7:])), WORKSPACE,
          'workspace')
  refused(lib.vtc_jfif_unstuff_bytes(*(un[:7] + [need - 1] + un[8:])),
          WORKSPACE, 'workspace')
  overlap = ctypes.c_void_p(p[0].value + 4999)
  refused(lib.vtc_jfif_unstuff_bytes(*(un[:2] + [overlap] + un[3:])), INVALID,
          'overlaps')

  unpack = [p[0], 1000, p[1], p[2], 6, p[3], p[4], p[5], p[6], p[7], 10, p[8],
            p[9], 1 << 20, null]
  need = lib.vtc_jfif_unpack_workspace_bytes(1000)
  assert need > 0 and lib.vtc_jfif_unpack_workspace_bytes(0) == 0
  assert lib.vtc_jfif_unpack_workspace_bytes(32769) > need   # a second group
  for i in (0, 2, 3, 5, 6, 7, 8, 9, 11):
    refused(lib.vtc_jfif_unpack(*(unpack[:i] + [null] + unpack[i + 1:])),
            INVALID, 'vtc_jfif_unpack', 'null')
  for i, bad, word in ((1, 0, 'seg_bytes'), (1, 1 << 31, 'seg_bytes'),
                       (4, 0, 'nslots'), (4, 11, 'nslots'), (10, 0, 'rows')):
    refused(lib.vtc_jfif_unpack(*(unpack[:i] + [bad] + unpack[i + 1:])),
            INVALID, 'bad size ' + word)
  refused(lib.vtc_jfif_unpack(*(unpack[:12] + [null] + unpack[13:])),
          WORKSPACE, 'workspace')
  refused(lib.vtc_jfif_unpack(*(unpack[:13] + [need - 1] + unpack[14:])),
          WORKSPACE, 'workspace')

  dc = [p[0], 300, p[1], p[2], p[3], 1 << 20, null]
  need = lib.vtc_jfif_dc_accumulate_workspace_bytes(300)
  assert need == 2 * 256 and lib.vtc_jfif_dc_accumulate_workspace_bytes(0) == 0
  for i in (0, 2, 3):
    refused(lib.vtc_jfif_dc_accumulate(*(dc[:i] + [null] + dc[i + 1:])),
            INVALID, 'vtc_jfif_dc_accumulate', 'null')
  refused(lib.vtc_jfif_dc_accumulate(*(dc[:1] + [0] + dc[2:])), INVALID,
          'bad size d')
  refused(lib.vtc_jfif_dc_accumulate(*(dc[:4] + [null] + dc[5:])), WORKSPACE,
          'workspace')
  refused(lib.vtc_jfif_dc_accumulate(*(dc[:5] + [need - 1] + dc[6:])),
          WORKSPACE, 'workspace')


# ------------------------------------------------------------ parse_headers
def _check_against_the_restatement(data):
  jfif = _jfif()
  got = jfif.parse_headers(data)
  want = truth.decode(data)
  assert got['shape'] == want['shape']
  assert data[got['segment_at'] - 3:got['segment_at']] == b'\x00\x3f\x00'
  if len(got['components']) == 1:
    assert got['sampling'] == [(1, 1)]
  else:
    assert got['sampling'] == want['sampling']
  assert len(got['qtables']) == len(want['qtables'])
  assert all(np.array_equal(got['qtables'][k], q) for k, q in zip(
      sorted(got['qtables']), want['qtables']))
  for pair in got['tables']:
    if pair is None:
      continue
    for key, size in (('dc', 16), ('ac', 256)):
      assert pair[key].shape == (size,) and pair[key + '_codes'].shape == (
          size,)
      # these encoders list the symbols of a length in ascending order
      assert np.array_equal(jfif.canonical_codes(pair[key])[0],
                            pair[key + '_codes'])
  return got


def test_parse_headers_on_the_restatements_files():
  for image, sub in ((truth.gray_image(17, 23), None),
                     (truth.colour_image(33, 19), (1, 1)),
                     (truth.colour_image(33, 19), (2, 2))):
    if sub is None:
      data, info = truth.encode_gray(image, 75)
    else:
      data, info = truth.encode_rgb(image, sub, 75)
    got = _check_against_the_restatement(data)
    assert got['segment_at'] == info['header_bytes'] - 2
    assert got['selectors'] == [(c['td'], c['td']) for c in info['comps']]
    assert [c[3] for c in got['components']] == [c['tq']
                                                 for c in info['comps']]
    for pair, table in zip(got['tables'], info['tables']):
      assert (pair is None) == (table is None)
      if pair is not None:
        assert np.array_equal(pair['dc'], table['dc'])
        assert np.array_equal(pair['ac'], table['ac'])


def test_parse_headers_on_the_foreign_files():
  files = dd.load_foreign()
  assert sorted(files) == sorted(dd.FOREIGN)
  want = {'gray': [(1, 1)], '444': [(1, 1)] * 3,
          '422': [(2, 1), (1, 1), (1, 1)], '420': [(2, 2), (1, 1), (1, 1)],
          '420-default-tables': [(2, 2), (1, 1), (1, 1)]}
  for name, data in files.items():
    assert 1000 < len(data) < 4096
    got = _check_against_the_restatement(data)
    assert got['shape'] == (64, 96) and got['sampling'] == want[name], name
  longest = max(int(t['ac'].max()) for t in _jfif().parse_headers(
      files['420-default-tables'])['tables'])
  assert longest == 16


# ------------------------------------------------------------- frame_layout
@pytest.mark.parametrize('shape,sub', [((17, 23), None), ((8, 8), None),
                                       ((33, 19), (1, 1)), ((33, 19), (2, 2)),
                                       ((64, 48), (2, 2))])
def test_frame_layout_is_scan_layout_where_that_knows_the_case(shape, sub):
  jfif = _jfif()
  old = jfif.scan_layout(shape, sub)
  sampling = [(1, 1)] if sub is None else [(sub[1], sub[0]), (1, 1), (1, 1)]
  new = jfif.frame_layout(shape, sampling)
  assert sorted(set(new) - set(old)) == ['order', 'start']
  for key, value in old.items():
    if isinstance(value, list) and value and isinstance(value[0], np.ndarray):
      assert all(np.array_equal(a, b) and a.dtype == b.dtype
                 for a, b in zip(value, new[key])), key
    elif isinstance(value, np.ndarray):
      assert np.array_equal(value, new[key]) and value.dtype == new[key].dtype
    else:
      assert value == new[key], key
  # order walks each component's pred chain
  order, start = new['order'], new['start']
  assert order.dtype == np.int32 and start.dtype == np.uint8
  assert sorted(order.tolist()) == list(range(new['rows']))
  for j, row in enumerate(order):
    assert new['pred'][row] == (-1 if start[j] else order[j - 1])


def test_frame_layout_17x23_at_422_and_440_by_hand():
  jfif = _jfif()
  lay = jfif.frame_layout((17, 23), [(2, 1), (1, 1), (1, 1)])   # 4:2:2
  # MCU 8 rows x 16 columns: 3 x 2 MCUs of Y0 Y1 Cb Cr
  assert lay['rows'] == 24 and lay['subsampling'] == (1, 2)
  assert lay['plane_shapes'] == [(17, 23), (17, 12), (17, 12)]
  assert lay['grids'] == [(3, 4), (3, 2), (3, 2)]
  assert lay['component'].tolist() == [0, 0, 1, 2] * 6
  assert lay['row_of_block'][0].reshape(3, 4).tolist() == [
      [0, 1, 4, 5], [8, 9, 12, 13], [16, 17, 20, 21]]
  assert lay['row_of_block'][1].tolist() == [2, 6, 10, 14, 18, 22]
  assert lay['row_of_block'][2].tolist() == [3, 7, 11, 15, 19, 23]
  assert lay['pred'].tolist() == [
      -1, 0, -1, -1, 1, 4, 2, 3, 5, 8, 6, 7, 9, 12, 10, 11, 13, 16, 14, 15,
      17, 20, 18, 19]
  assert lay['order'].tolist() == [0, 1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21,
                                   2, 6, 10, 14, 18, 22,
                                   3, 7, 11, 15, 19, 23]
  assert lay['start'].nonzero()[0].tolist() == [0, 12, 18]

  lay = jfif.frame_layout((17, 23), [(1, 2), (1, 1), (1, 1)])   # 4:4:0
  # MCU 16 rows x 8 columns: 2 x 3 MCUs of Y0 (top) Y1 (bottom) Cb Cr
  assert lay['rows'] == 24 and lay['subsampling'] == (2, 1)
  assert lay['plane_shapes'] == [(17, 23), (9, 23), (9, 23)]
  assert lay['grids'] == [(4, 3), (2, 3), (2, 3)]
  assert lay['row_of_block'][0].reshape(4, 3).tolist() == [
      [0, 4, 8], [1, 5, 9], [12, 16, 20], [13, 17, 21]]
  assert lay['row_of_block'][1].tolist() == [2, 6, 10, 14, 18, 22]
  assert lay['order'].tolist() == [0, 1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21,
                                   2, 6, 10, 14, 18, 22,
                                   3, 7, 11, 15, 19, 23]
  with pytest.raises(NotImplementedError):
    jfif.frame_layout((17, 23), [(4, 1), (1, 1), (1, 1)])
  with pytest.raises(NotImplementedError):
    jfif.frame_layout((17, 23), [(2, 2), (2, 1), (1, 1)])
  with pytest.raises(ValueError):
    jfif.frame_layout((0, 23), [(1, 1)])


# ---------------------------------------------------------------- refusals
YCC = ((1, 2, 2, 0), (2, 1, 1, 0), (3, 1, 1, 0))
UNSUPPORTED = {
    'progressive': (dict(sof=0xC2), 'progressive'),
    'extended sequential': (dict(sof=0xC1), 'SOF1'),
    'arithmetic': (dict(sof=0xC9), 'arithmetic'),
    'lossless': (dict(sof=0xC3), 'lossless'),
    '12-bit': (dict(precision=12), '12-bit'),
    'DRI': (dict(extra=dd.segment(0xDD, b'\x00\x04')), 'restart'),
    '16-bit DQT': (dict(dqt=((1, 0),)), '16-bit DQT'),
    'DHT id 2': (dict(tables=((0, 0), (1, 0), (0, 2))), 'table ids'),
    'spectral selection': (dict(spectral=(0, 5, 0)), 'Ss, Se'),
    'successive approximation': (dict(spectral=(0, 63, 1)), 'Ah/Al'),
    'a scan of one component': (dict(components=YCC, scan_components=[1]),
                                'all components'),
    'a scan in another order': (dict(components=YCC,
                                     scan_components=[2, 1, 3]),
                                'all components'),
    'four components': (dict(components=YCC + ((4, 1, 1, 0),)),
                        '4 components'),
    'two components': (dict(components=YCC[:2]), '2 components'),
    'luma 4 x 1': (dict(components=((1, 4, 1, 0),) + YCC[1:]),
                   'luma sampling'),
    'chroma 2 x 1': (dict(components=(YCC[0], (2, 2, 1, 0), YCC[2])),
                     'chroma sampling'),
    'Adobe RGB': (dict(components=YCC, extra=dd.segment(
        0xEE, b'Adobe\x00\x64\x00\x00\x00\x00\x00')), 'Adobe'),
    'scan table id 2': (dict(scan_tables=[(2, 0)]), 'table ids'),
}


@pytest.mark.parametrize('name', sorted(UNSUPPORTED))
def test_parse_headers_names_what_it_leaves_out(name):
  jfif = _jfif()
  kwargs, word = UNSUPPORTED[name]
  with pytest.raises(NotImplementedError, match=re.escape(word)):
    jfif.parse_headers(dd.header_file(**kwargs))


def test_parse_headers_accepts_the_plain_files():
  jfif = _jfif()
  got = jfif.parse_headers(dd.header_file())
  assert got['shape'] == (8, 8) and got['selectors'] == [(0, 0)]
  assert got['tables'][1] is None and got['tables'][0]['dc'][0] == 1
  got = jfif.parse_headers(dd.header_file(components=YCC, h=16, w=16))
  assert got['sampling'] == [(2, 2), (1, 1), (1, 1)]
  # an Adobe segment that says YCbCr, fill bytes in front of a marker, a
  # comment, and a one-component file that states 2 x 2 sampling
  adobe = dd.segment(0xEE, b'Adobe\x00\x64\x00\x00\x00\x00\x01')
  got = jfif.parse_headers(dd.header_file(
      components=YCC, extra=adobe + b'\xff\xff' + dd.segment(0xFE, b'hello')))
  assert got['shape'] == (8, 8)
  got = jfif.parse_headers(dd.header_file(components=((7, 2, 2, 0),)))
  assert got['sampling'] == [(1, 1)] and got['components'] == [(7, 2, 2, 0)]


def test_parse_headers_value_errors():
  jfif = _jfif()
  good = dd.header_file()
  jfif.parse_headers(good)
  for bad in (b'', b'\x89PNG\r\n\x1a\n', good[1:], b'\xff\xd8',
              b'\xff\xd8\xff\xd9', good[:20], good[:2] + b'\x00' + good[2:]):
    with pytest.raises(ValueError):
      jfif.parse_headers(bad)
  # every prefix that ends before the segment is truncated, never an
  # IndexError
  at = jfif.parse_headers(good)['segment_at']
  for cut in range(2, at):
    with pytest.raises(ValueError):
      jfif.parse_headers(good[:cut])
  parts = dd.header_parts
  cases = {
      'missing DC table': parts(tables=((1, 0),)),
      'missing AC table': parts(tables=((0, 0),)),
      'scan refers to pair 1': parts(scan_tables=[(1, 1)]),
      'missing DQT': parts(dqt=()),
      'component refers to table 1': parts(components=((1, 1, 1, 1),)),
      'SOS before SOF': [s for s in parts() if s[:2] != b'\xff\xc0'],
      'DHT class 2': parts(tables=((0, 0), (1, 0), (2, 0))),
      'zero width': parts(w=0),
  }
  for name, segments in cases.items():
    with pytest.raises(ValueError):
      jfif.parse_headers(b''.join(segments) + b'\x3f\xff\xd9')
      pytest.fail(name + ' was accepted')
  # a DHT whose lengths overflow the code space, and one naming a symbol twice
  for counts, values in (([3] + [0] * 15, [0, 1, 2]),
                         ([0, 2] + [0] * 14, [5, 5])):
    segments = parts()
    segments.insert(-1, dd.segment(0xC4, bytes([0x10]) + bytes(counts) +
                                   bytes(values)))
    with pytest.raises(ValueError):
      jfif.parse_headers(b''.join(segments) + b'\x3f\xff\xd9')


def test_pil_progressive_and_restart_files_are_refused():
  Image = pytest.importorskip('PIL.Image')
  jfif = _jfif()
  picture = Image.fromarray(dd.foreign_image())
  buf = io.BytesIO()
  picture.save(buf, format='JPEG', quality=85, progressive=True)
  with pytest.raises(NotImplementedError, match='progressive'):
    jfif.parse_headers(buf.getvalue())
  buf = io.BytesIO()
  picture.save(buf, format='JPEG', quality=85, restart_marker_blocks=2)
  assert b'\xff\xdd' in buf.getvalue()
  with pytest.raises(NotImplementedError, match='restart'):
    jfif.parse_headers(buf.getvalue())
  # and a baseline file from PIL passes
  buf = io.BytesIO()
  picture.save(buf, format='JPEG', quality=85)
  assert jfif.parse_headers(buf.getvalue())['shape'] == (64, 96)


# ------------------------------------------------------- the restatements
def test_the_sequential_decoder_opens_the_foreign_files():
  """The truth of tests/test_jfif_decode_gpu.py for constructed segments,
  held here to the restatement's own decoder on whole files."""
  jfif = _jfif()
  for name, data in dd.load_foreign().items():
    hdr = jfif.parse_headers(data)
    lay = jfif.frame_layout(hdr['shape'], hdr['sampling'])
    seg, marker_at = dd.unstuff(data[hdr['segment_at']:])
    assert data[hdr['segment_at'] + marker_at:] == b'\xff\xd9'
    arrays = {
        key: np.stack([np.zeros(size, dtype) if t is None else np.asarray(
            t[field]).astype(dtype) for t in hdr['tables']])
        for key, field, size, dtype in (
            ('ac_code', 'ac_codes', 256, np.uint16),
            ('ac_len', 'ac', 256, np.uint8),
            ('dc_code', 'dc_codes', 16, np.uint16),
            ('dc_len', 'dc', 16, np.uint8))}
    slot_dc, slot_ac = jfif._slots(lay, hdr['selectors'])
    levels, status = dd.sequential_unpack(seg, slot_dc, slot_ac, arrays,
                                          lay['rows'])
    assert status[:2] == [0, lay['rows']] and 0 <= 8 * len(seg) - status[2] < 8
    levels = dd.dc_accumulate(levels, lay['order'], lay['start'])
    assert np.array_equal(levels, truth.decode(data)['levels']), name


def test_python_refusals():
  torch = pytest.importorskip('torch')
  import vtc_hip
  jfif = _jfif()
  with pytest.raises(vtc_hip.VtcHipError):
    jfif.unstuff_bytes(torch.zeros(4, dtype=torch.uint8))
  with pytest.raises(vtc_hip.VtcHipError):
    jfif.unpack_scan(torch.zeros(4, dtype=torch.uint8), dd.one_table_layout(1),
                     [None, None])
  with pytest.raises(vtc_hip.VtcHipError):
    jfif.dc_accumulate(torch.zeros((1, 64), dtype=torch.int32),
                       dd.one_table_layout(1))
  with pytest.raises(ValueError):
    jfif.decode_bytes(b'not a jpeg')
  with pytest.raises(NotImplementedError):
    jfif.decode_bytes(dd.header_file(sof=0xC2))
  # refused on the host, before any device work: no EOI, a restart marker,
  # another marker behind the segment
  good = dd.header_file()
  for tail, word in ((b'\x3f', 'truncated'), (b'\x3f\xff', 'truncated'),
                     (b'\x3f\xff\xd0\x3f\xff\xd9', 'restart'),
                     (b'\x3f\xff\xda', 'EOI')):
    with pytest.raises(ValueError, match=word):
      jfif.decode_bytes(good[:-3] + tail)
