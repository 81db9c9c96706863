"""The numpy mirror of the trajectory renderer (visualization.render_trajectories_numpy, the definition of gcpx_topdown_trajectories):
the state -> pixel arithmetic against a literal float32 restatement of multiroom3d_env.py:163-170, the raster against an independent
per-pixel test in exact rationals and against pixel sets typed out by hand, the paint order, the segment colours, and what happens to
NaN, +-Inf and 1e30 states.  No GPU."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import video_gcp_amd  # noqa: E402,F401
from video_gcp_amd import dataset as DS  # noqa: E402
from video_gcp_amd import image_log as IL  # noqa: E402
from video_gcp_amd import visualization as V  # noqa: E402
import topdown_fixture as TF  # noqa: E402

RED, GREEN = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)


def _assets(arrays):
    a = dict(background=arrays["background"], cw=int(arrays["crop_window"]), n_rooms=int(arrays["n_rooms"]),
             scale=int(arrays["render_scale"]), agent_stamp=arrays["agent_stamp"], goal_stamp=arrays["goal_stamp"],
             agent_color=arrays["agent_color"], goal_color=arrays["goal_color"])
    a["S"] = int(DS.topdown_table_size(a["n_rooms"]) * a["scale"])
    return a


def _small(k=5, seed=3):
    """a 24 x 24 picture (9 rooms at scale 24) with asymmetric k x k stamps"""
    a = _assets(TF.make_assets(seed=seed, n_rooms=9, scale=24, cw=4, k=k))
    assert a["S"] == 24
    return a


def _states(a, pix):
    """states whose pixels in the unpadded picture are `pix` (the fixture works in the padded one)"""
    pix = np.asarray(pix).reshape(-1, 2)
    st = TF.states_for_pixels(pix + a["cw"], a["n_rooms"], a["scale"], a["S"], a["cw"])
    got, ok = V.trajectory_pixels(st, a["n_rooms"], a["scale"], a["S"])
    assert ok.all() and np.array_equal(got, np.clip(pix, -V.TRAJ_COORD_LIMIT, V.TRAJ_COORD_LIMIT)), (got, pix)
    return st


def _layer(states, color=RED, dim_t=None, length=None):
    st = np.asarray(states, dtype=np.float32)[None]
    return dict(states=st, length=np.array([st.shape[1] if length is None else length]), color=color,
                dim_t=None if dim_t is None else np.asarray(dim_t, dtype=np.int32)[None])


# ---- pixel arithmetic ---------------------------------------------------------------------------------------------------------------
def _restated_pixels(traj, n_rooms, scale, S):
    """multiroom3d_env.py:163-170 on a float32 array, every operation in float32"""
    table_size = (1 / 3) * int(math.sqrt(n_rooms))
    traj = np.array(traj, dtype=np.float32).copy()
    traj = traj[:, :2]
    traj[:, 1] *= -1
    if traj.max() > 1.0 or traj.min() < -1.0:
        traj = traj / np.float32(27.0)
    traj = traj + np.float32(0.5 * table_size)
    return [(int(traj[i, 0] * np.float32(scale)), S - int(traj[i, 1] * np.float32(scale))) for i in range(traj.shape[0])]


@pytest.mark.parametrize("n_rooms,scale", [(9, 256), (25, 256), (9, 50), (25, 31)])
def test_pixels_equal_the_float32_restatement(n_rooms, scale):
    S = int((1 / 3) * int(math.sqrt(n_rooms)) * scale)
    rng = np.random.RandomState(n_rooms + scale)
    inside = rng.uniform(-1, 1, size=(40, 2)).astype(np.float32)            # max <= 1 and min >= -1: no division
    outside = rng.uniform(-13.5, 13.5, size=(40, 2)).astype(np.float32)      # divided by 27
    edge = np.array([[1.0, -1.0], [0.25, 0.5]], dtype=np.float32)           # exactly 1 and -1: still no division
    over = np.array([[0.5, -1.0000001], [0.25, 0.5]], dtype=np.float32)     # the flipped y is the maximum, just above 1
    uncentred = (rng.uniform(-40, 60, size=(60, 2)) + 7.3).astype(np.float32)
    for traj, divided in ((inside, False), (outside, True), (edge, False), (over, True), (uncentred, True)):
        flipped = traj * np.array([1, -1], dtype=np.float32)
        assert bool(flipped.max() > 1.0 or flipped.min() < -1.0) == divided
        got, ok = V.trajectory_pixels(traj, n_rooms, scale, S)
        assert ok.all() and got.tolist() == [list(p) for p in _restated_pixels(traj, n_rooms, scale, S)]
    # the y flip by hand: 9 rooms at 256: (13.5, -13.5) is the top right corner, x = 256 and y = 256 - int(1.0 * 256) = 0
    got, _ = V.trajectory_pixels(np.array([[13.5, -13.5], [-13.5, 13.5], [0, 0]], dtype=np.float32), 9, 256, 256)
    assert got.tolist() == [[256, 0], [0, 256], [128, 128]]
    # without the division the same numbers are render units themselves: (0.25, -0.5) -> x = int(0.75 * 256), y = 256 - int(1.0 * 256)
    got, _ = V.trajectory_pixels(np.array([[0.25, -0.5], [0, 0]], dtype=np.float32), 9, 256, 256)
    assert got.tolist() == [[192, 0], [128, 128]]


# ---- raster -------------------------------------------------------------------------------------------------------------------------
def _near(a, b, q, half=2):
    """q within `half` of the segment a -> b: the closest point of the segment in exact rationals"""
    d = (b[0] - a[0], b[1] - a[1])
    dd = d[0] * d[0] + d[1] * d[1]
    t = Fraction(0) if dd == 0 else min(max(Fraction((q[0] - a[0]) * d[0] + (q[1] - a[1]) * d[1], dd), Fraction(0)), Fraction(1))
    cx, cy = a[0] + t * d[0], a[1] + t * d[1]
    return (q[0] - cx) ** 2 + (q[1] - cy) ** 2 <= half * half


def _brute(a, layers):
    """the spec applied pixel by pixel: layers = [(pixels [m, 2], ok [m], colours [m - 1, 3])]"""
    S, cw, k = a["S"], a["cw"], a["agent_stamp"].shape[0]
    img = a["background"][cw:cw + S, cw:cw + S].copy()
    for pix, ok, cols in layers:
        m = len(pix)
        for y in range(S):
            for x in range(S):
                for j in range(m - 1):
                    if ok[j] and ok[j + 1] and _near(tuple(int(v) for v in pix[j]), tuple(int(v) for v in pix[j + 1]), (x, y)):
                        img[y, x] = cols[j]
                for stamp, color, p in ((a["agent_stamp"], a["agent_color"], 0), (a["goal_stamp"], a["goal_color"], m - 1)):
                    dx, dy = x - int(pix[p][0]) + k // 2, y - int(pix[p][1]) + k // 2
                    if ok[p] and 0 <= dx < k and 0 <= dy < k and stamp[dy, dx]:
                        img[y, x] = color
    return img


def _line_pixels(a, pix):
    """the pixels one red polyline paints in red on a black picture without stamps"""
    a = dict(a, background=np.zeros_like(a["background"]), agent_stamp=np.zeros_like(a["agent_stamp"]),
             goal_stamp=np.zeros_like(a["goal_stamp"]))
    img = V.render_trajectories_numpy(a, [_layer(_states(a, pix))])[0]
    assert set(map(tuple, img.reshape(-1, 3).tolist())) <= {(0, 0, 0), (255, 0, 0)}
    ys, xs = np.nonzero(img[..., 0])
    return set(zip(xs.tolist(), ys.tolist()))


RASTER = dict(horizontal=[(5, 10), (9, 10)], vertical=[(10, 5), (10, 9)], diagonal=[(4, 4), (9, 9)], shallow=[(2, 3), (20, 8)],
              steep=[(15, 21), (13, 2)], same=[(6, 6), (6, 6)], far=[(3, 20), (500, -300)], corner=[(0, 0), (23, 23)],
              polyline=[(2, 2), (20, 4), (6, 18), (6, 7), (22, 22)])


@pytest.mark.parametrize("name", sorted(RASTER))
def test_raster_equals_the_per_pixel_test(name):
    a, pix = _small(), RASTER[name]
    got = V.render_trajectories_numpy(a, [_layer(_states(a, pix))])[0]
    cols = np.tile(np.array([[255, 0, 0]], dtype=np.uint8), (len(pix) - 1, 1))
    assert np.array_equal(got, _brute(a, [(pix, [True] * len(pix), cols)]))
    assert _line_pixels(a, pix) == _line_pixels(a, pix[::-1])              # the reversed end points paint the same pixels


def test_raster_typed_out():
    a = _small()
    rows = lambda spec: {(x, y) for y, (x0, x1) in spec.items() for x in range(x0, x1 + 1)}
    assert _line_pixels(a, [(5, 10), (9, 10)]) == rows({8: (5, 9), 9: (4, 10), 10: (3, 11), 11: (4, 10), 12: (5, 9)})
    assert _line_pixels(a, [(10, 5), (10, 9)]) == {(y, x) for x, y in rows({8: (5, 9), 9: (4, 10), 10: (3, 11), 11: (4, 10), 12: (5, 9)})}
    disk = rows({4: (6, 6), 5: (5, 7), 6: (4, 8), 7: (5, 7), 8: (6, 6)})   # the 13 pixels within 2 of (6, 6)
    assert _line_pixels(a, [(6, 6), (6, 6)]) == disk
    # a single point has no segment: only the two stamps, the goal's over the agent's
    img = V.render_trajectories_numpy(a, [_layer(_states(a, [(6, 6)]))])[0]
    want = a["background"][4:28, 4:28].copy()
    for stamp, color in ((a["agent_stamp"], a["agent_color"]), (a["goal_stamp"], a["goal_color"])):
        want[4:9, 4:9][stamp] = color
    assert np.array_equal(img, want)
    # the diagonal from (4, 4) to (8, 8): |dy - dx| <= 2 between the end points' normals, and the two disks
    diag = {(x, y) for x in range(24) for y in range(24) if abs((y - 4) - (x - 4)) <= 2 and 0 < (x - 4) + (y - 4) < 8}
    diag |= rows({2: (4, 4), 3: (3, 5), 4: (2, 6), 5: (3, 5), 6: (4, 4)}) | rows({6: (8, 8), 7: (7, 9), 8: (6, 10), 9: (7, 9), 10: (8, 8)})
    assert _line_pixels(a, [(4, 4), (8, 8)]) == diag


# ---- order --------------------------------------------------------------------------------------------------------------------------
def test_paint_order():
    a = _small()
    k = 5
    # one layer whose segment 3 crosses segment 1 and whose segment 1 is darker (dim_t = 2 halves segments 1 and 2)
    pix = [(2, 12), (8, 12), (20, 12), (20, 20), (14, 20), (14, 4)]
    img = V.render_trajectories_numpy(a, [_layer(_states(a, pix), dim_t=[2])])[0]
    assert img[12, 5].tolist() == [255, 0, 0] and img[12, 17].tolist() == [127, 0, 0]
    assert img[12, 8].tolist() == [127, 0, 0]                               # segment 1's round end over segment 0's
    assert img[12, 14].tolist() == [255, 0, 0] and img[12, 13].tolist() == [255, 0, 0]          # the later segment 4 over segment 1
    assert img[16, 20].tolist() == [127, 0, 0] and img[20, 17].tolist() == [255, 0, 0]
    cols = V.segment_colors(RED, 6, 6, [2])
    assert cols.tolist() == [[255, 0, 0], [127, 0, 0], [127, 0, 0], [255, 0, 0], [255, 0, 0]]
    assert np.array_equal(img, _brute(a, [(pix, [True] * 6, cols)]))
    # stamps over lines, the goal's stamp over the agent's: a short line whose stamps overlap
    pix = [(10, 10), (12, 11)]
    img = V.render_trajectories_numpy(a, [_layer(_states(a, pix))])[0]
    am, gm = np.zeros((24, 24), bool), np.zeros((24, 24), bool)
    am[8:13, 8:13], gm[9:14, 10:15] = a["agent_stamp"], a["goal_stamp"]
    assert (am & gm).any() and (am & ~gm).any()
    assert (img[gm] == a["goal_color"]).all() and (img[am & ~gm] == a["agent_color"]).all()
    line = np.array([[_near(pix[0], pix[1], (x, y)) for x in range(24)] for y in range(24)])
    assert (img[line & ~am & ~gm] == [255, 0, 0]).all() and (line & ~am & ~gm).any()
    rest = ~(line | am | gm)
    assert np.array_equal(img[rest], a["background"][4:28, 4:28][rest])
    # a swapped stamp or a transposed one cannot pass: the fixture's stamps differ from each other and from their transposes
    assert not np.array_equal(a["agent_stamp"], a["goal_stamp"]) and not np.array_equal(a["agent_stamp"], a["agent_stamp"].T)
    # layer 2's line over layer 1's stamps
    g, r = [(3, 12), (20, 12)], [(20, 12), (3, 13)]
    img = V.render_trajectories_numpy(a, [_layer(_states(a, g), GREEN), _layer(_states(a, r), RED)])[0]
    green_agent = np.zeros((24, 24), bool)
    green_agent[10:15, 1:6] = a["agent_stamp"]
    red_goal = np.zeros((24, 24), bool)
    red_goal[11:16, 1:6] = a["goal_stamp"]
    red_line = np.array([[_near(r[0], r[1], (x, y)) for x in range(24)] for y in range(24)])
    over = green_agent & red_line & ~red_goal
    assert over.any() and (img[over] == [255, 0, 0]).all()
    assert img[12, 11].tolist() == [255, 0, 0] and img[10, 11].tolist() == [0, 255, 0]
    ones = [True, True]
    assert np.array_equal(img, _brute(a, [(g, ones, np.array([[0, 255, 0]], np.uint8)), (r, ones, np.array([[255, 0, 0]], np.uint8))]))
    assert k == a["agent_stamp"].shape[0]


# ---- colours ------------------------------------------------------------------------------------------------------------------------
def test_segment_colours():
    # duplicates (2 twice), a value above len - 1 (9 -> 6), t = 0 (its t - 1 wraps to the unused last entry); 2 and 3 both hit segment 2
    assert V.segment_colors(RED, 7, 7, [2, 3, 2, 9, 0]).tolist() == [[127, 0, 0], [127, 0, 0], [63, 0, 0], [127, 0, 0], [255, 0, 0],
                                                                      [127, 0, 0]]
    assert V.segment_colors(RED, 7, 7, None).tolist() == [[255, 0, 0]] * 6
    assert V.segment_colors(RED, 4, 4, [0, 0, 0]).tolist() == [[127, 0, 0], [255, 0, 0], [255, 0, 0]]      # once per distinct t
    assert V.segment_colors(RED, 4, 4, [3]).tolist() == [[255, 0, 0], [255, 0, 0], [127, 0, 0]]            # only through t - 1
    assert V.segment_colors((0.5, 1.0, 0.2), 3, 3, [1]).tolist() == [[63, 127, 25]] * 2                    # trunc(c * 0.5 * 255)
    assert V.segment_colors(GREEN, 1, 1, [0]).shape == (0, 3)
    # m < len (a states tensor shorter than the sequence): the clamp is to len - 1, beyond every segment
    assert V.segment_colors(RED, 3, 9, [7, 20]).tolist() == [[255, 0, 0]] * 2
    # through the renderer: the colour of every segment's middle pixel
    a = _small()
    pix = [(2, 2), (8, 2), (14, 2), (20, 2), (20, 9), (20, 16), (20, 22)]
    img = V.render_trajectories_numpy(a, [_layer(_states(a, pix), dim_t=[2, 3, 2, 9, 0])])[0]
    mids = [(5, 2), (11, 2), (17, 2), (20, 6), (20, 13), (20, 19)]
    assert [int(img[y, x, 0]) for x, y in mids] == [127, 127, 63, 127, 255, 127]
    assert all(img[y, x, 1] == 0 and img[y, x, 2] == 0 for x, y in mids)


# ---- states that are not numbers -------------------------------------------------------------------------------------------------------
def test_non_finite_and_huge_states():
    a = _small()
    S, scale = a["S"], a["scale"]
    base = _states(a, [(3, 3), (10, 4), (12, 15), (18, 18), (21, 6)])
    red = lambda m: np.tile(np.array([[255, 0, 0]], np.uint8), (m - 1, 1))
    with np.errstate(all="raise"):                                           # no warning escapes either
        # NaN: numpy's max / min return it, so nothing is divided: the other points are render units themselves
        st = base.copy()
        st[2, 0] = np.nan
        pix, ok = V.trajectory_pixels(st, 9, scale, S)
        assert ok.tolist() == [True, True, False, True, True]
        half = np.float32(0.5)
        want = [[int((np.float32(x) + half) * np.float32(scale)), S - int((np.float32(-y) + half) * np.float32(scale))]
                for x, y in st[[0, 1, 3, 4]].tolist()]
        assert np.clip(want, -V.TRAJ_COORD_LIMIT, V.TRAJ_COORD_LIMIT).tolist() == pix[[0, 1, 3, 4]].tolist()
        img = V.render_trajectories_numpy(a, [_layer(st)])[0]
        assert np.array_equal(img, _brute(a, [(pix, ok, red(5))]))           # segments 1 and 2 are skipped
        # +-Inf: the maximum is Inf, everything is divided; the infinite point is skipped, the others are where they were
        for v, p in ((np.inf, 0), (-np.inf, 4), (np.inf, 2)):
            st = base.copy()
            st[p, 1] = v
            pix, ok = V.trajectory_pixels(st, 9, scale, S)
            assert ok.tolist() == [i != p for i in range(5)]
            keep = [i for i in range(5) if i != p]
            assert pix[keep].tolist() == V.trajectory_pixels(base, 9, scale, S)[0][keep].tolist()
            img = V.render_trajectories_numpy(a, [_layer(st)])[0]
            assert np.array_equal(img, _brute(a, [(pix, ok, red(5))]))       # also: no stamp on a skipped first / last point
        # 1e30 is finite after the arithmetic: clamped to the coordinate limit, the segments towards it are drawn
        st = base.copy()
        st[2] = (1e30, 1e30)
        pix, ok = V.trajectory_pixels(st, 9, scale, S)
        assert ok.all() and pix[2].tolist() == [V.TRAJ_COORD_LIMIT, V.TRAJ_COORD_LIMIT]
        st[2] = (-1e30, 1e30)
        pix, ok = V.trajectory_pixels(st, 9, scale, S)
        assert ok.all() and pix[2].tolist() == [-V.TRAJ_COORD_LIMIT, V.TRAJ_COORD_LIMIT]
        img = V.render_trajectories_numpy(a, [_layer(st)])[0]
        assert np.array_equal(img, _brute(a, [(pix, ok, red(5))]))
        # 3e38 / 27 * 256 overflows float32 (at this picture's scale of 24 it does not): not finite, skipped
        st[2] = (3e38, 0)
        assert V.trajectory_pixels(st, 9, 256, 256)[1].tolist() == [True, True, False, True, True]
        assert V.trajectory_pixels(st, 9, scale, S)[1].all()
        # every point NaN, and a length of 0: only the background
        img = V.render_trajectories_numpy(a, [_layer(np.full((3, 2), np.nan)), _layer(base, length=0)])[0]
        assert np.array_equal(img, a["background"][4:28, 4:28])
    # the int64 test cannot overflow at the limits: the largest cross product squared, times 4
    lim, far = V.TRAJ_COORD_LIMIT, 2048 + 32
    assert 4 * (2 * (2 * lim) * (lim + far)) ** 2 < 2 ** 63


def test_lengths_and_batches():
    """per-canvas lengths (1, 2 and all points), a length beyond the states (numpy truncates the slice), two canvases"""
    a = _small(seed=4)
    pix = np.array([[(2, 2), (9, 5), (15, 20), (21, 3)], [(20, 20), (4, 18), (5, 5), (12, 12)], [(1, 22), (22, 1), (11, 3), (3, 11)]])
    st = np.stack([_states(a, p) for p in pix])
    for lengths in ([1, 2, 4], [9, 3, 1]):
        img = V.render_trajectories_numpy(a, [dict(states=st, length=np.array(lengths), color=GREEN, dim_t=None)])
        for i, ln in enumerate(lengths):
            m = min(ln, 4)
            want = _brute(a, [(pix[i][:m], [True] * m, np.tile(np.array([[0, 255, 0]], np.uint8), (m - 1, 1)))])
            assert np.array_equal(img[i], want), (lengths, i)


# ---- --log_images 0 -------------------------------------------------------------------------------------------------------------------
def test_no_panel_without_log_images():
    """with log_images false a model that holds a nav dataset's assets builds nothing: no renderer, no launch, no file"""
    class Model:
        topdown_assets = _small()
        log_dir = "/nonexistent"
        lib = None

    def panels(*args):
        raise AssertionError("no panel may be asked for")

    m = Model()
    assert IL.log_outputs(m, panels, None, None, None, 0, False, "train") == []
    assert "_image_log_panels" not in m.__dict__ and not hasattr(m, "last_panels")
    assert IL.trajectory_renderer(type("Plain", (), {})()) is None          # a model without assets has no renderer at all


def test_constants_equal_the_header():
    """the mirror's constants are the export's (include/gcpx.h)"""
    import re
    text = open(os.path.join(ROOT, "include", "gcpx.h")).read()
    val = lambda name: int(re.search(r"^#define " + name + r" (\d+)$", text, re.M).group(1))
    assert V.TRAJ_THICKNESS == val("GCPX_TRAJ_THICKNESS") and V.TRAJ_COORD_LIMIT == val("GCPX_TRAJ_COORD_LIMIT")
