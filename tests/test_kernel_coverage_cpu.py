"""A ledger of which C-ABI entry points of include/gcpx.h the GPU suite calls directly (no GPU, no library load: the test reads files).

Every `int gcpx_*(` declaration must be either
  (a) called in some tests/test_gpu_*.py — `.gcpx_name(` on the library handle, or passed as `lib.gcpx_name`; or
  (b) listed in INFRASTRUCTURE with a reason: it has no arithmetic of its own to compare with a reference.
INDIRECT used to list the entry points whose only cover was a model-level test (whole-model outputs or parameter gradients at 1e-3 of a
tensor's max-abs).  It is empty and asserted to stay empty: the backward kernels have their kernel-level tests in
tests/test_gpu_backward_kernels.py and tests/test_gpu_kernels.py, the forward / planner glue in tests/test_gpu_glue_kernels.py, the
adaptive-binding kernels in tests/test_gpu_adaptive_kernels.py, the loss, KL and BatchNorm-statistics kernels in
tests/test_gpu_loss_kernels.py (references and bounds: tests/loss_refs.py, pinned by tests/test_loss_refs_cpu.py), the optimizer and
gradient-clip kernels in tests/test_gpu_optim_kernels.py (tests/optim_refs.py, pinned by tests/test_optim_refs_cpu.py).  A new entry
point needs a direct test or an INFRASTRUCTURE reason.
Being called is no cover for an entry point that dispatches to many device bodies: the exact row GEMM behind gcpx_gemm (28 gemm_tile
bodies, csrc/gemm_tile.h) has every one of them asserted through gcpx_gemm_form and held to float64 in tests/test_gpu_gemm_forms.py
(tests/gemm_refs.py, pinned by tests/test_gemm_refs_cpu.py); the encoder convs behind gcpx_conv4x4s2 and gcpx_conv4x4s2_image (three
direct, five LDS, five split-f16 and three image bodies, csrc/conv_enc.hip and csrc/conv_enc_split.hip, the LDS and split ones at every
frames-per-block choice that changes a workgroup's work) are asserted through gcpx_conv4x4s2_form / gcpx_conv4x4s2_image_form and held
to float64 in tests/test_gpu_enc_forms.py (tests/enc_refs.py, pinned by tests/test_enc_refs_cpu.py)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INFRASTRUCTURE = {
    "gcpx_version": "ABI version query (checked by build())",
    "gcpx_conv_grid": "grid-size query",
    "gcpx_gemm_form": "dispatch query",
    "gcpx_conv4x4s2_form": "dispatch query", "gcpx_conv4x4s2_image_form": "dispatch query",
    "gcpx_graph_begin": "hipGraph capture", "gcpx_graph_end": "hipGraph capture", "gcpx_graph_launch": "hipGraph replay",
    "gcpx_graph_destroy": "hipGraph handle",
    "gcpx_stream_create": "stream handle", "gcpx_stream_create_priority": "stream handle", "gcpx_stream_destroy": "stream handle",
    "gcpx_stream_wait_event": "stream ordering",
    "gcpx_event_create": "event handle", "gcpx_event_create_sync": "event handle", "gcpx_event_record": "event handle",
    "gcpx_event_elapsed_ms": "event timing", "gcpx_event_destroy": "event handle",
}

INDIRECT = {}

# entry points the backward pass launches for their arithmetic: never acceptable in INDIRECT
BACKWARD = ("_bwd", "gcpx_wgrad", "gcpx_colsum", "gcpx_reduce_partials", "gcpx_tree_accum", "gcpx_timestep_scatter", "gcpx_add_rows",
            "gcpx_rows_strided", "gcpx_zero_unmapped_rows", "gcpx_index_offset", "gcpx_index_inverse", "gcpx_col2im4x4s2", "gcpx_im2col_image",
            "gcpx_conv_stage", "gcpx_gemm_group")


def _declared():
    with open(os.path.join(ROOT, "include", "gcpx.h")) as f:
        names = re.findall(r"^int (gcpx_\w+)\(", f.read(), re.M)
    assert len(names) > 100 and len(set(names)) == len(names), "include/gcpx.h: declarations not found / duplicated"
    return names


def _gpu_test_sources():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))
    assert files
    text = ""
    for p in files:
        with open(p) as f:
            text += f.read() + "\n"
    return text


def _called(name, text):
    return re.search(r"\." + name + r"\b", text) is not None


def test_every_entry_point_is_called_by_a_gpu_test_or_listed():
    names, text = _declared(), _gpu_test_sources()
    missing = [n for n in names if not _called(n, text) and n not in INFRASTRUCTURE and n not in INDIRECT]
    assert not missing, (f"no tests/test_gpu_*.py calls {missing}: add a kernel-level test, or, for an entry point without arithmetic of its "
                         "own, list the name in INFRASTRUCTURE with the reason")


def test_no_entry_point_is_covered_only_indirectly():
    assert not INDIRECT, f"{sorted(INDIRECT)}: a model-level test is no cover for an entry point: call it directly in a tests/test_gpu_*.py"


def test_the_tables_are_current():
    names, text = _declared(), _gpu_test_sources()
    both = set(INFRASTRUCTURE) & set(INDIRECT)
    assert not both, f"listed twice: {sorted(both)}"
    for n in list(INFRASTRUCTURE) + list(INDIRECT):
        assert n in names, f"{n} is listed but include/gcpx.h does not declare it"
    stale = [n for n in INDIRECT if _called(n, text)]
    assert not stale, f"{stale} now have a direct call in a GPU test: remove them from INDIRECT"
    for n, ref in INDIRECT.items():
        path, _, test = ref.partition("::")
        with open(os.path.join(ROOT, path)) as f:
            assert re.search(r"^def " + re.escape(test) + r"\(", f.read(), re.M), f"{n}: {ref} does not exist"


def test_no_backward_kernel_is_covered_only_indirectly():
    bad = [n for n in list(INDIRECT) + list(INFRASTRUCTURE) if any(k in n for k in BACKWARD) and not n.endswith(("_blocks", "_dims", "_grid"))]
    assert not bad, f"backward-pass kernels need a kernel-level test of their own: {bad}"
