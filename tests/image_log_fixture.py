"""Shared by the picture-log tests: the golden cases of tests/golden/ref_image_log.npz as (panel, sources, expected canvas), and the
tests' own PNG / APNG decoder (zlib + filter type 0 only)."""
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_image_log.npz")
L, RES, T, B = 3, 8, 7, 4


def golden_cases():
    """[(case name, visualization.Panel, {source: numpy array}, expected f32 canvas [n, H, W, 3], frames kept)]"""
    from video_gcp_amd import visualization as V
    g = np.load(GOLDEN)
    src = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    for level in range(L):                       # the per-level layout of the attention weights: row b * 2^level + j
        ids = [(2 * j + 1) * 2 ** (L - 1 - level) - 1 for j in range(2 ** level)]
        src[f"gamma{level}"] = np.ascontiguousarray(src["gamma_df"][:, ids]).reshape(B * 2 ** level, T)
    assert src["node_t"].dtype == np.int32 and src["end_ind"].dtype == np.int64 and src["pruned_len"].dtype == np.int32
    ns = min(V.N_LOGGED_SEQS, B)
    first = lambda k: np.ascontiguousarray(g["out_" + k].transpose(0, 2, 3, 1))      # [n, C, H, W] -> [n, H, W, C]
    cases = [
        ("hs_plain", V.hierarchical_splits(L, RES, T), first("hs_plain")),
        ("hs_full", V.hierarchical_splits(L, RES, T, attentive=True, dense=True, soft=True), first("hs_full")),
        ("match_overview", V.match_overview("match_overview", L, RES, T, attr="match_dist", soft=True), g["out_match_overview"]),
        ("attention_masks", V.match_overview("attention_masks", L, RES, T, attr="gamma", soft=True), g["out_attention_masks"]),
        ("output_tree", V.output_tree(L, RES, T), g["out_output_tree"]),
        ("pruned_seq_gif", V.rows_gif("pruned_seq_gif", RES, [("pruned_padded", T, "pruned_len")], ns, T), first("pruned_seq_gif")),
        ("gt_target_gif_train", V.rows_gif("gt_target_gif", RES, [("traj_seq", T, None), ("soft", T, None)], ns, T),
         first("gt_target_gif_train")),
        ("gt_target_gif_val", V.rows_gif("gt_target_gif", RES, [("soft", T, None)], ns, T), first("gt_target_gif_val")),
        ("dense_rec_train", V.rows_gif("dense_rec", RES, [("traj_seq", T, None), ("dense_rec", T, None)], ns, T),
         first("dense_rec_train")),
        ("dense_rec_val", V.rows_gif("dense_rec", RES, [("dense_rec", T, None)], ns, T), first("dense_rec_val")),
    ]
    out = []
    for name, panel, want in cases:
        keep = int(src["pruned_len"].max()) if name == "pruned_seq_gif" else panel.n       # pad_sequence: the longest sequence
        out.append((name, panel, src, np.asarray(want, np.float32), keep))
    return out


def decode_png(data):
    """(frames uint8 [n, H, W, 3], delays in seconds per frame or [] for a still) of an 8-bit RGB PNG / APNG with filter-0 rows"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1][0] == b"IEND"
    W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0)
    streams, delays, n_frames, seq = [], [], 1, 0
    for tag, body in chunks[1:-1]:
        if tag == b"acTL":
            n_frames = struct.unpack(">II", body)[0]
        elif tag == b"fcTL":
            s, w, h, x, y, num, den, _, _ = struct.unpack(">IIIIIHHBB", body)
            assert (s, w, h, x, y) == (seq, W, H, 0, 0)
            seq += 1
            delays.append(num / den)
        elif tag == b"IDAT":
            streams.append(body)
        elif tag == b"fdAT":
            assert struct.unpack(">I", body[:4])[0] == seq
            seq += 1
            streams.append(body[4:])
    assert len(streams) == n_frames
    frames = []
    for s in streams:
        raw = np.frombuffer(zlib.decompress(s), np.uint8).reshape(H, 1 + W * 3)
        assert not raw[:, 0].any(), "only filter type 0 is written"
        frames.append(raw[:, 1:].reshape(H, W, 3))
    return np.stack(frames), delays
