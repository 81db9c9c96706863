"""Picture logs (video-gcp_amd/visualization.py, image_log.py) without a GPU: the numpy restatement of every panel against canvases
the reference's own logger computed (tests/golden/ref_image_log.npz, written by tests/golden/make_ref_image_log_goldens.py) exactly,
the PNG / APNG writer through the test's own decoder and through Pillow, log_outputs with the pictures off, the trainer's flags, and
the new export's declaration, binding, struct layout and argument checks."""
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd  # noqa: E402,F401
from video_gcp_amd import image_log as IL  # noqa: E402
from video_gcp_amd import visualization as V  # noqa: E402
import image_log_fixture as FX  # noqa: E402

CASES = FX.golden_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_numpy_panels_equal_the_reference_canvases_exactly(case):
    """copies, (x + 1) / 2 in f32 and the gamma strips added in depth-first order: equality, not a tolerance"""
    name, panel, src, want, keep = case
    got = V.compose(panel, src)[:keep]
    assert got.dtype == np.float32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (name, int((got != want).sum()), float(np.abs(got - want).max()))


def test_the_golden_tree_has_the_collision_the_step_0_node_and_the_masked_tail():
    _, panel, src, want, _ = CASES[1]                    # hs_full
    node_t, end_ind = src["node_t"], src["end_ind"]
    assert node_t[0, 1] == node_t[0, 5] and node_t[0, 0] == 0 and (end_ind < FX.T - 1).any()
    res, lh = FX.RES, FX.RES + V.GAMMA_WIDTH
    # level 1 of sample 0, step 2: the later node of the depth-first order (5) is the one drawn
    tile = want[0, res + lh + V.GAMMA_WIDTH:res + 2 * lh, 2 * res:3 * res]
    later, earlier = [(src["images_df"][0, i].transpose(1, 2, 0) + np.float32(1)) / np.float32(2) for i in (5, 1)]
    assert np.array_equal(tile, later) and not np.array_equal(tile, earlier)
    # the dense-rec row of sample 1 (end_ind 4): frames 5 and 6 are x * 0 -> 0.5
    r = res + FX.L * lh
    assert (want[1, r:r + res, 5 * res:] == 0.5).all() and not (want[1, r:r + res, 4 * res:5 * res] == 0.5).all()


def test_uint8_is_truncation_of_the_clipped_canvas():
    x = np.array([-0.3, 0.0, 0.5, 0.999, 1.0, 1.7, 1 / 255, 254.999 / 255], np.float32)
    assert V.to_uint8(x).tolist() == [0, 0, 127, 254, 255, 255, 1, 254]


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


@pytest.mark.parametrize("n", [1, 5])
def test_png_and_apng_round_trip(n, tmp_path):
    rng = np.random.RandomState(n)
    frames = rng.randint(0, 256, size=(n, 18, 33, 3)).astype(np.uint8)
    path = IL.write_png(str(tmp_path / "sub" / ("a.apng" if n > 1 else "a.png")), frames if n > 1 else frames[0])
    data = open(path, "rb").read()
    got, delays = FX.decode_png(data)
    assert got.shape == frames.shape and np.array_equal(got, frames)
    assert delays == ([] if n == 1 else [1 / V.FPS] * n) and V.FPS == 4
    assert (b"acTL" in data) == (n > 1) and data.count(b"IDAT") == 1
    Image = _pil()
    if Image is not None:                                # (the check above has already run: this only adds a second reader)
        im = Image.open(io.BytesIO(data))
        assert im.size == (33, 18) and getattr(im, "n_frames", 1) == n
        for i in range(n):
            im.seek(i)
            assert np.array_equal(np.asarray(im.convert("RGB")), frames[i]), i
            if n > 1:
                assert im.info.get("duration") == 1000 / V.FPS


class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"log_outputs(log_images=False) read .{name}")

    __getitem__ = __getattr__


@pytest.mark.parametrize("cls", ["model.GCPTreeModel", "sequential.GCPSequentialModel"])
def test_log_outputs_with_pictures_off_touches_nothing(cls, tmp_path, monkeypatch):
    import importlib
    mod, name = cls.split(".")
    klass = getattr(importlib.import_module("video_gcp_amd." + mod), name)
    model = object.__new__(klass)                        # no device, no library: the call must not need either
    monkeypatch.chdir(tmp_path)
    assert klass.log_outputs(model, _Untouchable(), _Untouchable(), _Untouchable(), 0, False, "train") == []
    assert klass.log_outputs(model, _Untouchable(), _Untouchable(), _Untouchable(), 0, 0, "val") == []
    assert os.listdir(tmp_path) == [] and "_image_log_panels" not in model.__dict__


def test_trainer_flags():
    from video_gcp_amd.train import get_cmd_args
    a = get_cmd_args([])
    assert a.log_images == 0 and a.imepoch == 4
    a = get_cmd_args(["--log_images", "1", "--imepoch", "2"])
    assert a.log_images == 1 and a.imepoch == 2


def test_tile_table_names_slots_in_first_use_order():
    panel = V.hierarchical_splits(FX.L, FX.RES, FX.T, attentive=True, soft=True)
    tab, names = IL.tile_table(panel)
    assert names[:2] == ["traj_seq", "gamma2"] and len(names) <= 16 and len(tab) == len(panel.tiles)
    node = [d for d in tab if d.index >= 0][0]
    assert names[node.index] == "node_t" and node.index_stride == 7 and node.index_count == FX.T and names[node.src] == "images_df"
    soft = tab[len(panel.tiles) - 1]
    assert names[soft.length] == "end_ind" and soft.flags == V.LENGTH_I64 and soft.nf == FX.T


def test_constants_and_struct_layout_match_the_header(tmp_path):
    from video_gcp_amd import runtime as rt
    src = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "gcpx.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu\n", sizeof(gcpx_panel_tile), offsetof(gcpx_panel_tile, tile_w), offsetof(gcpx_panel_tile, index_off),
             offsetof(gcpx_panel_tile, fill), offsetof(gcpx_panel_tile, off));
      printf("%d %d %d %d %d %d %d %d %d %d\n", GCPX_PANEL_MAX_SRCS, GCPX_PANEL_IMAGE, GCPX_PANEL_GREY, GCPX_PANEL_GREY_ADD,
             GCPX_PANEL_FILL, GCPX_PANEL_RESCALE, GCPX_PANEL_LENGTH_STRICT, GCPX_PANEL_INDEX_FRAME, GCPX_PANEL_INDEX_I64,
             GCPX_PANEL_LENGTH_I64);
      return 0;
    }'''
    c = tmp_path / "t.c"
    c.write_text(src)
    exe = str(tmp_path / "t")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    P = rt.PanelTile
    want = [C.sizeof(P), P.tile_w.offset, P.index_off.offset, P.fill.offset, P.off.offset, rt.PANEL_MAX_SRCS, rt.PANEL_IMAGE,
            rt.PANEL_GREY, rt.PANEL_GREY_ADD, rt.PANEL_FILL, rt.PANEL_RESCALE, rt.PANEL_LENGTH_STRICT, rt.PANEL_INDEX_FRAME,
            rt.PANEL_INDEX_I64, rt.PANEL_LENGTH_I64]
    assert got == want, (got, want)
    assert (V.IMAGE, V.GREY, V.GREY_ADD, V.FILL) == (rt.PANEL_IMAGE, rt.PANEL_GREY, rt.PANEL_GREY_ADD, rt.PANEL_FILL)
    assert (V.RESCALE, V.LENGTH_STRICT, V.INDEX_FRAME, V.INDEX_I64, V.LENGTH_I64) == (
        rt.PANEL_RESCALE, rt.PANEL_LENGTH_STRICT, rt.PANEL_INDEX_FRAME, rt.PANEL_INDEX_I64, rt.PANEL_LENGTH_I64)


def test_invalid_arguments_are_rejected_without_a_gpu():
    from video_gcp_amd import runtime as rt
    lib = rt.load_library()
    f = C.c_float(0.7)
    buf = (C.c_uint8 * 64)()
    assert lib.gcpx_panel_compose(None, 1, None, None, 0, 1, 1, 1, f, 0, None, buf, None) == -1          # tiles without a table
    assert b"gcpx_panel_compose" in lib.gcpx_last_error()
    assert lib.gcpx_panel_compose(None, 0, None, None, 0, 1, 1, 1, f, 0, None, None, None) == -1          # no canvas
    assert lib.gcpx_panel_compose(None, 0, None, None, 17, 1, 1, 1, f, 0, None, buf, None) == -1          # too many sources
    assert lib.gcpx_panel_compose(None, 0, None, None, 0, 0, 1, 1, f, 0, None, buf, None) == -1           # empty canvas
    assert lib.gcpx_panel_compose(None, 0, None, None, 0, 1, 1, 1, f, 0, None, C.byref(buf, 1), None) == -1   # misaligned canvas
