"""The ledger of tests/test_gpu_store_bounds.py: every entry point of the C ABI (_lib.SIGNATURES) either has a guarded case there, or
is listed here as writing no device memory, with the reason.  A new entry point fails this test until it gets one or the other."""
import os
import re

from collision_handling_in_instantngp_amd import _lib

import test_gpu_store_bounds as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WRITES_NOTHING = {
    "gngf_abi_version": "returns a constant",
    "gngf_encode_bwd_bucketed_plan": "host arithmetic: fills a host array of six integers",
    "gngf_set_tiled_interleaved": "sets a process-wide host switch",
    "gngf_tiled_interleaved_applies": "host logic only, no launch",
    "gngf_debug_il_stamps": "copies device-side cycle stamps to a HOST array (and clears the library's own static counters)",
    "gngf_decoder_bwd_last_span_ns": "reads the library's own device-side time stamps into a HOST double",
    "gngf_decoder_hidden_floats": "size query",
    "gngf_decoder_bwd_slabs": "size query",
    "gngf_decoder_slab_floats": "size query",
    "gngf_set_decoder_bwd_hybrid": "sets a process-wide host switch",
    "gngf_hpd_bwd_fused_applies": "host logic only, no launch",
    "gngf_mse_workspace_floats": "size query",
    "gngf_mse_blocks": "size query",
    "gngf_js_kl_workspace_doubles": "size query",
    "gngf_slot_bitmap_words": "size query",
    "gngf_adam_block_elems": "size query",
    "gngf_image_metrics_blocks": "size query",
    "gngf_image_metrics_workspace_words": "size query",
    "gngf_epoch_state_bytes": "size query",
    "gngf_epoch_log_int_columns": "size query",
    "gngf_snapshot_block_bytes": "size query",
}

# guarded elsewhere: entry point -> (test file, test name)
GUARDED_ELSEWHERE = {
    "gngf_snapshot_if": ("test_gpu_epoch_loop.py", "test_snapshot_if_copies_exactly_its_bytes_or_nothing"),
}


def test_every_entry_point_has_a_case_or_a_reason():
    covered = set(sb.entry_points())
    names = set(_lib.SIGNATURES)
    assert covered <= names, f"cases for entry points the binding does not know: {sorted(covered - names)}"
    assert set(WRITES_NOTHING) <= names and set(GUARDED_ELSEWHERE) <= names
    missing = names - covered - set(WRITES_NOTHING) - set(GUARDED_ELSEWHERE)
    assert not missing, f"no store-bounds case and no reason for: {sorted(missing)}"
    twice = (covered & set(WRITES_NOTHING)) | (covered & set(GUARDED_ELSEWHERE)) | (set(WRITES_NOTHING) & set(GUARDED_ELSEWHERE))
    assert not twice, f"listed twice: {sorted(twice)}"
    assert all(isinstance(why, str) and why.strip() for why in WRITES_NOTHING.values())


def test_entry_points_listed_as_writing_nothing_take_no_device_output():
    """what the header declares: none of them has a non-const pointer parameter other than a host array (`plan`, `ns`, `host8`)"""
    with open(os.path.join(ROOT, "include", "gngf.h")) as f:
        header = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    host_outputs = {"plan", "ns", "host8"}
    for name in WRITES_NOTHING:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/gngf.h"
        for param in [p.strip() for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]:
            if "*" in param and not param.startswith("const "):
                assert param.split("*")[-1].strip() in host_outputs, f"{name} takes a writable pointer: {param}"


def test_the_test_it_points_to_exists_and_guards_its_output():
    for name, (path, test) in GUARDED_ELSEWHERE.items():
        with open(os.path.join(ROOT, "tests", path)) as f:
            text = f.read()
        assert f"def {test}(" in text, f"{name}: {path} has no {test}"
        body = text.split(f"def {test}(")[1].split("\ndef ")[0]
        assert "guard" in body, f"{name}: {test} no longer speaks of guard words"


def test_case_table_is_plain_data_with_unique_ids():
    ids = [sb.case_id(c) for c in sb.CASE_TABLE]
    assert len(ids) == len(set(ids)), sorted(i for i in set(ids) if ids.count(i) > 1)[:5]
    for entry, label, runner, kw in sb.CASE_TABLE:
        assert entry.startswith("gngf_") and label and runner in sb.RUNNERS and isinstance(kw, dict)
        assert entry in sb.case_id((entry, label, runner, kw)) and label in sb.case_id((entry, label, runner, kw))
