"""CPU checks of the scalar logs (video_gcp_amd/scalar_log.py): the event-file format read back by a reader written here from the
format's description alone, scalar_data.json, the segment / chunk tables of gcpx_grad_segment_norms, its numpy mirror against float64,
and the argument checks of the two entry points."""
import ctypes as C
import json
import os
import re
import struct

import numpy as np
import pytest

from video_gcp_amd import scalar_log as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


# ---- an independent reader: CRC-32C bit by bit, TFRecord framing, the protobuf wire format ----
def _crc32c_bitwise(data):
    c = 0xFFFFFFFF
    for b in data:
        c ^= b
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    return c ^ 0xFFFFFFFF


def _mask(c):
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) % 2 ** 32


def _read_varint(buf, i):
    v, shift = 0, 0
    while True:
        b = buf[i]
        i += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return v, i


def _fields(buf):
    """[(field number, wire type, value)] of one message"""
    out, i = [], 0
    while i < len(buf):
        key, i = _read_varint(buf, i)
        f, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _read_varint(buf, i)
        elif wt == 1:
            v, i = buf[i:i + 8], i + 8
        elif wt == 2:
            n, i = _read_varint(buf, i)
            v, i = buf[i:i + n], i + n
        elif wt == 5:
            v, i = buf[i:i + 4], i + 4
        else:
            raise AssertionError(f"wire type {wt}")
        out.append((f, wt, v))
    return out


def read_event_file(path):
    """[dict(wall_time, step, file_version | tag + value)] -- every record's two checksums verified"""
    data, i, events = open(path, "rb").read(), 0, []
    while i < len(data):
        (n,) = struct.unpack("<Q", data[i:i + 8])
        assert struct.unpack("<I", data[i + 8:i + 12])[0] == _mask(_crc32c_bitwise(data[i:i + 8]))
        payload = data[i + 12:i + 12 + n]
        assert len(payload) == n
        assert struct.unpack("<I", data[i + 12 + n:i + 16 + n])[0] == _mask(_crc32c_bitwise(payload))
        i += 16 + n
        ev = {"step": 0}
        for f, wt, v in _fields(payload):
            if (f, wt) == (1, 1):
                ev["wall_time"] = struct.unpack("<d", v)[0]
            elif (f, wt) == (2, 0):
                ev["step"] = v - 2 ** 64 if v >= 2 ** 63 else v
            elif (f, wt) == (3, 2):
                ev["file_version"] = v.decode()
            elif (f, wt) == (5, 2):
                (vf, vwt, val), = _fields(v)                  # Summary: one `value`
                assert (vf, vwt) == (1, 2)
                for g, gwt, gv in _fields(val):
                    if (g, gwt) == (1, 2):
                        ev["tag"] = gv.decode()
                    elif (g, gwt) == (2, 5):
                        ev["value"] = struct.unpack("<f", gv)[0]
                    else:
                        raise AssertionError((g, gwt))
            else:
                raise AssertionError((f, wt))
        events.append(ev)
    return events


def test_crc32c_rfc3720_vectors():
    assert SL.crc32c(bytes(32)) == 0x8A9136AA
    assert SL.crc32c(b"123456789") == 0xE3069283
    assert SL.crc32c(bytes([0xFF] * 32)) == 0x62A8AB43 and SL.crc32c(bytes(range(32))) == 0x46DD794E       # RFC 3720 B.4, too
    for d in (b"", b"a", bytes(range(256))):
        assert SL.crc32c(d) == _crc32c_bitwise(d)
        assert SL.masked_crc32c(d) == _mask(_crc32c_bitwise(d))


def test_event_file_round_trip(tmp_path):
    log = SL.ScalarLogger(str(tmp_path / "events"))
    want = [("kl_loss", "train", 0, 1.5), ("kl_loss", "train", 10, np.float32(0.1)), ("gradients/mean_norm", "train", 10, 3e-7),
            ("total_loss", "val", 300, -2.25), ("kl_loss_layerwise/level_3", "val", 2 ** 40 + 5, float("nan")),
            ("dense_img_rec_loss", "train", -1, float("inf")), ("x" * 200, "val", 127, 1e30), ("y", "val", 128, 0.0)]
    for name, phase, step, v in want:
        log.log_scalar(v, name, step, phase)
    log.flush()
    files = os.listdir(tmp_path / "events")
    assert len(files) == 1 and re.fullmatch(r"events\.out\.tfevents\.\d{10}\..+", files[0])
    ev = read_event_file(log.event_path)                     # readable after a flush, before close
    log.close()
    assert ev[0].get("file_version") == "brain.Event:2" and "tag" not in ev[0] and ev[0]["wall_time"] > 1e9
    assert len(ev) == 1 + len(want)
    for e, (name, phase, step, v) in zip(ev[1:], want):
        assert e["tag"] == f"{name}_{phase}" and e["step"] == step and "file_version" not in e
        assert np.array_equal(np.float32(e["value"]), np.float32(v), equal_nan=True)
        assert e["wall_time"] >= ev[0]["wall_time"]
    assert len(read_event_file(log.event_path)) == len(ev)                  # closing adds nothing


def test_scalar_data_json_shape(tmp_path):
    log = SL.ScalarLogger(str(tmp_path / "events"))
    for step in (0, 10):
        for name in ("dense_img_rec", "kl"):
            log.log_scalar(0.5 + step, name + "_loss", step, "train")
        log.log_scalar(np.float32(0.3), "gradients/mean_norm", step, "train")
    log.log_scalar(2.0, "kl_loss", 20, "val")
    path = log.dump_scalars()
    log.close()
    assert path == str(tmp_path / "events" / "scalar_data.json") and sorted(os.listdir(tmp_path / "events")) == sorted(
        ["scalar_data.json", os.path.basename(log.event_path)])
    d = json.load(open(path))
    assert set(d) == {"dense_img_rec_loss_train", "kl_loss_train", "gradients/mean_norm_train", "kl_loss_val"}
    assert [r[1:] for r in d["kl_loss_train"]] == [[0, 0.5], [10, 10.5]] and d["kl_loss_val"][0][1:] == [20, 2.0]
    assert d["gradients/mean_norm_train"][1][2] == float(np.float32(0.3))
    for rows in d.values():
        for wall, step, value in rows:
            assert isinstance(wall, float) and wall > 1e9 and isinstance(step, int) and isinstance(value, float)


def _poffs():
    """the layouts of c1 and of the sequential model, without a device: offsets as WeightsMixin._flatten_params lays them out"""
    import video_gcp_amd as V
    res = {}
    for name, sd in (("c1", V.init_params(V.config("c1"), seed=0)),
                     ("seq", V.init_params_sequential(V.config("c1", nz_mid_lstm=128, lstm_init="zero"), seed=0))):
        off, poff = 0, {}
        for k, v in sd.items():
            poff[k] = (off, tuple(v.shape))
            off += (v.numel() + 3) // 4 * 4
        res[name] = (poff, off)
    return res


def test_layout_assumed_here_is_the_models():
    """_poffs restates _flatten_params: hold the two together by source (the model itself needs a device)"""
    src = open(os.path.join(ROOT, "video-gcp_amd", "weights.py")).read()
    assert "self._poff[k] = (off, tuple(v.shape))" in src and "off += (v.numel() + 3) // 4 * 4" in src


@pytest.mark.parametrize("which", ["c1", "seq"])
def test_segment_and_chunk_tables(which):
    poff, total = _poffs()[which]
    names, chunks, seg0 = SL.grad_tables(poff)
    assert chunks.dtype.itemsize == 16 and seg0.dtype == np.int32
    params = [k for k in poff if not k.endswith(("running_mean", "running_var"))]
    assert names == params and len(params) < len(poff) and not [n for n in names if "running_" in n]
    assert len(seg0) == len(names) + 1 and seg0[0] == 0 and seg0[-1] == len(chunks) and (np.diff(seg0) >= 1).all()
    cover = np.zeros(total, np.int32)                 # how many chunks hold each float of the flat vector
    for s, name in enumerate(names):
        off, shape = poff[name]
        numel = int(np.prod(shape))
        cs = chunks[seg0[s]:seg0[s + 1]]
        assert (cs["seg"] == s).all()                  # the chunks of a segment are adjacent
        assert (cs["length"] >= 1).all() and (cs["length"] <= SL.GRAD_NORM_CHUNK).all()
        assert cs["first"][0] == off and (cs["first"][1:] == cs["first"][:-1] + cs["length"][:-1]).all()
        assert cs["first"][-1] + cs["length"][-1] == off + numel            # no chunk crosses its segment's end
        assert (cs["first"] % 4 == 0).all()            # 16-byte loads everywhere
        for c in cs:
            cover[c["first"]:c["first"] + c["length"]] += 1
    want = np.zeros(total, np.int32)
    for name in names:
        off, shape = poff[name]
        want[off:off + int(np.prod(shape))] = 1
    assert np.array_equal(cover, want)                # every counted element exactly once; padding and buffers never
    assert want.sum() < total


def test_kernel_constants_agree_with_the_header():
    text = open(os.path.join(ROOT, "include", "gcpx.h")).read()
    get = lambda n: re.search(r"#define " + n + r" (.+)", text).group(1).strip()
    assert int(get("GCPX_GRAD_NORM_THREADS")) == SL.GRAD_NORM_THREADS and int(get("GCPX_GRAD_NORM_CHUNK")) == SL.GRAD_NORM_CHUNK
    assert get("GCPX_GRAD_NORM_SERIAL") == "(GCPX_GRAD_NORM_CHUNK / GCPX_GRAD_NORM_THREADS + 1)"
    assert SL.GRAD_NORM_SERIAL == SL.GRAD_NORM_CHUNK // SL.GRAD_NORM_THREADS + 1
    assert int(get("GCPX_GRAD_NORM_TREE_DEPTH")) == SL.GRAD_NORM_TREE_DEPTH == 8


def synthetic_segments(rng, lengths, zero=(), inf_at=None):
    """a flat vector of segments on 16-byte boundaries with NaN in every padding slot; -> (grad, poff)"""
    poff, off = {}, 0
    for i, n in enumerate(lengths):
        poff[f"p{i}.weight"] = (off, (n,))
        off += (n + 3) // 4 * 4
        if i == 2:                                    # a buffer in between: left out by name
            poff["bn.running_mean"] = (off, (5,))
            off += 8
    g = np.full(off, np.nan, np.float32)
    for i, n in enumerate(lengths):
        o = poff[f"p{i}.weight"][0]
        g[o:o + n] = 0 if i in zero else (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3)).astype(np.float32)
    g[poff["bn.running_mean"][0]:][:5] = 7.0
    if inf_at is not None:
        g[poff[f"p{inf_at}.weight"][0]] = np.inf
    return g, poff


def float64_norms(g, poff, names, mul=1.0):
    norms = np.array([np.sqrt(np.sum(g[poff[k][0]:poff[k][0] + int(np.prod(poff[k][1]))].astype(np.float64) ** 2)) * mul for k in names])
    counted = np.array([bool(np.any(g[poff[k][0]:poff[k][0] + int(np.prod(poff[k][1]))] != 0)) for k in names])
    return norms, counted


def test_numpy_mirror_against_float64():
    rng = np.random.default_rng(0)
    lengths = [1, 2, 3, 4, 5, 6, 7, 64, 1000, 16384, 16385, 40001, 3, 9]
    g, poff = synthetic_segments(rng, lengths, zero=(8,), inf_at=12)
    names, chunks, seg0 = SL.grad_tables(poff)
    assert len(names) == len(lengths)
    norm, stats = SL.segment_norms_numpy(g, chunks, seg0, grad_scale=0.5, coef=0.25)
    ref, counted = float64_norms(g, poff, names, 0.125)
    assert counted.sum() == len(lengths) - 1 and not counted[8] and norm[8] == 0
    # the mirror rounds a product and a sum where the kernel's fmaf rounds once: (2 S + D + 2) / 2 roundings on a norm
    bound = 0.5 * (2 * SL.GRAD_NORM_SERIAL + SL.GRAD_NORM_TREE_DEPTH + 2) * U
    fin = np.isfinite(ref)
    assert list(np.nonzero(~fin)[0]) == [12] and np.isinf(norm[12])              # the inf poisons its own segment only
    assert np.all(np.abs(norm[fin] - ref[fin]) <= bound * ref[fin])
    assert stats[2] == len(lengths) - 1 and stats[3] == 1 and np.isinf(stats[0]) and np.isinf(stats[1])
    # without the inf: mean and max
    g[poff["p12.weight"][0]] = 1.0
    norm, stats = SL.segment_norms_numpy(g, chunks, seg0)
    ref, counted = float64_norms(g, poff, names)
    assert np.all(np.abs(norm - ref) <= bound * ref) and stats[3] == 0 and stats[2] == counted.sum()
    assert abs(stats[0] - ref[counted].mean()) <= 2 * bound * ref[counted].mean() and abs(stats[1] - ref.max()) <= bound * ref.max()
    # a NaN inside a segment: its norm is NaN, the maximum keeps it (torch.max), two non-finite norms with the inf
    g[poff["p3.weight"][0] + 1], g[poff["p12.weight"][0]] = np.nan, np.inf
    norm, stats = SL.segment_norms_numpy(g, chunks, seg0)
    assert np.isnan(norm[3]) and np.isnan(stats[1]) and np.isnan(stats[0]) and stats[3] == 2
    # a clip coefficient of 0 means none
    assert np.array_equal(SL.segment_norms_numpy(g, chunks, seg0, 1.0, 0.0)[0], norm, equal_nan=True)


def test_invalid_args_are_rejected_without_a_gpu():
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    f = C.c_float(1.0)
    ok = dict(grad=p, n=16, chunks=p, n_chunks=2, seg0=p, n_seg=2, scale=f, coef=None, partial=p, n_partial=4, norm=p, stats=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gcpx_grad_segment_norms(a["grad"], a["n"], a["chunks"], a["n_chunks"], a["seg0"], a["n_seg"], a["scale"], a["coef"],
                                           a["partial"], a["n_partial"], a["norm"], a["stats"], None)
    for bad in (dict(grad=None), dict(chunks=None), dict(seg0=None), dict(partial=None), dict(norm=None), dict(stats=None), dict(n=0),
                dict(n_chunks=0), dict(n_seg=0), dict(n_seg=3), dict(n_partial=3), dict(grad=p + 2), dict(chunks=p + 4)):
        assert call(**bad) == -1, bad
        assert b"gcpx_grad_segment_norms" in lib.gcpx_last_error()

    def kl(qz=p, pz=p, B=1, L=2, nz=4, bs=24, ns=8, node_v=p, out=p):
        return lib.gcpx_kl_layerwise(qz, pz, B, L, nz, bs, ns, f, node_v, out, None)
    for bad in (dict(qz=None), dict(pz=None), dict(node_v=None), dict(out=None), dict(B=0), dict(L=0), dict(L=17), dict(nz=0), dict(nz=6),
                dict(bs=26), dict(ns=9), dict(qz=p + 4), dict(B=2 ** 20, L=16)):
        assert kl(**bad) == -1, bad
        assert b"gcpx_kl_layerwise" in lib.gcpx_last_error()
