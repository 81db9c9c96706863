"""The training guard without a GPU (video_gcp_amd/health.py): the numpy restatement of gcpx_grad_health against typed-out answers on a
hand-built table -- the bit patterns that must and must not count, gaps that are never read, the summary's fields -- and the flag."""
import numpy as np

from video_gcp_amd import health as H
from video_gcp_amd import scalar_log as SL


def _bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


def _table(segments):
    """chunks / seg_chunk0 of [(offset, length)] segments"""
    poff = {f"p{i}.weight": (off, (n,)) for i, (off, n) in enumerate(segments)}
    return SL.grad_tables(poff)


def test_bit_patterns_are_classified_by_exponent_mantissa_and_sign():
    x = _bits(0x7FC00000,      # quiet NaN
              0xFFC00000,      # quiet NaN, sign bit set
              0x7F800001,      # signalling NaN, smallest payload
              0xFF800001,      # the same with the sign bit
              0x7FFFFFFF,      # NaN, every payload bit
              0x7FA00000,      # signalling NaN, large payload
              0x7F800000,      # +Inf
              0xFF800000,      # -Inf
              0x7F7FFFFF,      # +FLT_MAX
              0xFF7FFFFF,      # -FLT_MAX
              0x00000001,      # smallest denormal
              0x807FFFFF,      # largest denormal, negative
              0x80000000,      # -0
              0x00000000,      # +0
              0x3F800000,      # 1
              0x00800000)      # FLT_MIN
    nan, pinf, ninf = H.classify_bits(x)
    assert list(nan) == [True] * 6 + [False] * 10
    assert list(pinf) == [False] * 6 + [True] + [False] * 9
    assert list(ninf) == [False] * 7 + [True] + [False] * 8
    names, chunks, seg0 = _table([(0, 16)])
    seg_bad, summary = H.health_numpy(x, chunks, seg0)
    assert seg_bad.tolist() == [[6, 1, 1]] and seg_bad.dtype == np.int32
    assert summary.tolist() == [6, 1, 1, 1, 0, 0, 1, 1] and summary.dtype == np.int32
    # the finite edge cases alone
    seg_bad, summary = H.health_numpy(x[8:], *_table([(0, 8)])[1:])
    assert seg_bad.tolist() == [[0, 0, 0]] and summary.tolist() == [0, 0, 0, 0, -1, 0, 0, 0]


def test_hand_built_table_with_nan_filled_gaps():
    # four segments at offsets 0, 4 (unaligned start at 5 below), 12, 20; every float between them is NaN and belongs to nobody
    x = np.full(32, np.nan, np.float32)
    segs = [(0, 3), (5, 4), (12, 5), (20, 9)]
    for off, n in segs:
        x[off:off + n] = 1.0
    names, chunks, seg0 = _table(segs)
    assert names == ["p0.weight", "p1.weight", "p2.weight", "p3.weight"] and seg0.tolist() == [0, 1, 2, 3, 4]
    seg_bad, summary = H.health_numpy(x, chunks, seg0)
    assert not seg_bad.any() and summary.tolist() == [0, 0, 0, 0, -1, 0, 0, 0]          # first bad is -1 on clean input
    x[5] = np.inf                       # first element of segment 1
    x[8] = -np.inf                      # its last
    x[16] = np.nan                      # last element of segment 2 (its len % 4 tail)
    x[20], x[28] = np.nan, np.inf       # first and last of segment 3
    seg_bad, summary = H.health_numpy(x, chunks, seg0, count0=4)
    assert seg_bad.tolist() == [[0, 0, 0], [0, 1, 1], [1, 0, 0], [1, 1, 0]]
    assert summary.tolist() == [2, 2, 1, 3, 1, 0, 1, 5]
    bad, ok = H.bad_list(names, seg_bad)
    assert bad == [("p1.weight", 0, 1, 1), ("p2.weight", 1, 0, 0), ("p3.weight", 1, 1, 0)] and ok == ["p0.weight"]


def test_extra_scalars_alone_set_the_verdict():
    x = np.ones(8, np.float32)
    names, chunks, seg0 = _table([(0, 8)])
    for extra, n_bad in ((np.float32([0.5, 2.0]), 0), (np.float32([0.5, np.nan]), 1), (np.float32([-np.inf, np.inf, 1.0]), 2),
                         (_bits(0x7F7FFFFF, 0x00000001), 0)):
        seg_bad, summary = H.health_numpy(x, chunks, seg0, extra=extra)
        assert not seg_bad.any() and summary.tolist() == [0, 0, 0, 0, -1, n_bad, int(n_bad > 0), int(n_bad > 0)]


def test_chunks_outside_the_vector_are_skipped_and_long_segments_are_cut():
    n = 2 * SL.GRAD_NORM_CHUNK + 7
    x = np.zeros(n + 1, np.float32)
    x[SL.GRAD_NORM_CHUNK - 1], x[SL.GRAD_NORM_CHUNK], x[n - 1] = np.nan, np.inf, -np.inf      # both sides of a seam, the tail
    names, chunks, seg0 = _table([(0, n)])
    assert len(chunks) == 3 and seg0.tolist() == [0, 3]
    seg_bad, summary = H.health_numpy(x, chunks, seg0)
    assert seg_bad.tolist() == [[1, 1, 1]] and summary[:5].tolist() == [1, 1, 1, 1, 0]
    bad = chunks.copy()
    bad["first"][2] = n                 # leaves the vector: not read, not counted
    seg_bad, _ = H.health_numpy(x, bad, seg0)
    assert seg_bad.tolist() == [[1, 1, 0]]


def test_weight_table_keeps_the_buffers():
    poff = {"a.weight": (0, (3,)), "bn.running_mean": (4, (2,)), "bn.running_var": (8, (2,)), "b.bias": (12, (1,))}
    assert SL.grad_tables(poff)[0] == ["a.weight", "b.bias"]
    names, chunks, seg0 = SL.grad_tables(poff, buffers=True)
    assert names == list(poff) and chunks["first"].tolist() == [0, 4, 8, 12] and chunks["length"].tolist() == [3, 2, 2, 1]


def test_the_flag_defaults_to_off():
    from video_gcp_amd.train import get_cmd_args
    assert get_cmd_args([]).nan_guard == "off"
    assert get_cmd_args(["--nan_guard", "raise"]).nan_guard == "raise" and get_cmd_args(["--nan_guard", "skip"]).nan_guard == "skip"


def test_the_exception_is_the_reference_s_value_error():
    e = H.NonFiniteGradients([("w", 0, 1, 0)], ["b"], 0)
    assert isinstance(e, ValueError) and str(e) == "there are NaN Gradients" and e.bad == [("w", 0, 1, 0)] and e.ok == ["b"]
