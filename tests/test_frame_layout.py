"""rayn_amd/csrc/frame_layout.h, the one definition of a worker's device memory layout: a dry carve() against the piece list restated here, the
per-path byte estimate and the 32-bit id limit.  CPU only: a stand-alone host program (tests/frame_layout_dump.cpp) prints what the header decides."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is absent")

SCAN_NC_BIN = 16
DTILE_BYTES = 32


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_layout") / "frame_layout_dump")
    subprocess.check_call([HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "frame_layout_dump.cpp"), "-o", exe])
    return lambda *args: subprocess.check_output([exe] + [str(a) for a in args], text=True)


def pieces(CAP, max_tiles, total_tiles, NS, max_bounces):
    """(name, element bytes, count) of every piece, written from the carve() that stood in rayn_hip.hip before the header existed (its tgbA / tgcA /
    tgbB / tgcB are ray_tgb / ray_tgc / bin_tgb / bin_tgc here; its flat Layout members are qt.*)."""
    QCAP = CAP + max_tiles * 64
    BCAP = CAP + max_tiles * (SCAN_NC_BIN * 3 + 64)
    JOBCAP = NS * BCAP
    QG, BG = QCAP // 64 + 1, BCAP // 64 + 1
    return [
        ("pool.geo0", 16, CAP), ("pool.geo1", 16, CAP), ("pool.col0", 16, CAP), ("pool.col1", 16, CAP), ("pool.aov", 16, CAP),
        ("pool.term_key", 4, CAP), ("pool.term_info", 1, CAP),
        ("q", 4, QCAP), ("qn", 4, QCAP), ("bq", 4, BCAP),
        ("qt.ent_obj", 1, QCAP), ("qt.alive", 8, BG),
        ("qt.grp_cnt", 1, QG * SCAN_NC_BIN), ("qt.grp_base", 4, QG * SCAN_NC_BIN), ("qt.grp_tile", 4, QG),
        ("qt.bgrp_cnt", 1, BG), ("qt.bgrp_base", 4, BG), ("qt.bgrp_tile", 4, BG),
        ("d_all_tiles", DTILE_BYTES, total_tiles), ("pgrp_tile", 4, CAP // 64 + 1),
        ("qt.ray_tgb", 4, max_tiles), ("qt.ray_tgc", 4, max_tiles), ("qt.bin_tgb", 4, max_tiles), ("qt.bin_tgc", 4, max_tiles),
        ("qt.tile_total", 4, max_tiles), ("qt.tile_valid", 4, max_tiles), ("qt.tile_out_base", 4, max_tiles),
        ("qt.tile_cls_cnt", 4, max_tiles * SCAN_NC_BIN), ("qt.tile_cls_base", 4, max_tiles * SCAN_NC_BIN),
        ("base_hist", 4, (max_bounces + 1) * max_tiles),
        ("nee.x", 4, 12 * BCAP), ("nee.vtr", 4, (NS - 4 + 1) * BCAP), ("nee.pdf", 4, NS * BCAP), ("nee.aux", 4, (NS - 4 + 1) * BCAP),
        ("nee.vis", 1, NS * BCAP), ("nee.vpicks", 8, BCAP),
        ("nee.T", 4, BCAP), ("nee.t0", 4, BCAP), ("nee.nthr", 4, 3 * BCAP), ("nee.flags", 1, BCAP),
        ("nee.job_ref", 4, JOBCAP), ("nee.job_geo", 8, 3 * JOBCAP),
    ], (QCAP, BCAP, BCAP, JOBCAP, max_tiles)


# the smallest layout (vtr / aux keep the one plane of NS - 4 + 1); a batch of more than 1024 tiles at the deepest frame; a batch of a larger share
SHAPES = [(64, 1, 1, 4, 0), (64 * 1281, 1280, 1280, 20, 120), (1 << 20, 3, 7, 12, 8)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_carve_matches_the_restated_pieces(dump, shape):
    want, caps = pieces(*shape)
    got = {}
    for line in dump("carve", *shape).splitlines():
        name, *vals = line.split()
        got[name] = [int(v) for v in vals]
    total, dry_total, got_caps = got.pop("total")[0], got.pop("dry_total")[0], tuple(got.pop("caps"))
    assert sorted(got) == sorted(n for n, _, _ in want)
    assert got_caps == caps
    need = {n: b * c for n, b, c in want}
    order = sorted(got, key=lambda n: got[n][0])
    ends = [got[n][0] for n in order[1:]] + [total]
    for n, end in zip(order, ends):
        off = got[n][0]
        assert off % 256 == 0, n
        assert end - off >= need[n], (n, off, end, need[n])  # at least its size, and the next piece begins behind it: no overlap
    assert got[order[0]][0] == 0
    assert total == dry_total == sum((v + 255) // 256 * 256 for v in need.values())


def test_bytes_per_path_is_the_estimate_render_device_used(dump):
    for NS in (4, 12, 16, 20):
        assert int(dump("per_path", NS)) == 118 + 81 + 33 * NS + 8 * (NS - 3)


def test_queue_ids_fit_at_both_limits(dump):
    limit = 2 ** 32 - 2 ** 26
    for NS in (4, 20):  # the product NS * slots
        assert int(dump("ids", NS, limit // NS)) == 1
        assert int(dump("ids", NS, limit // NS + 1)) == 0
    # the slot index: below 2^31 whatever the product (2^31 ids of one sample plane are fewer than the product's limit)
    assert int(dump("ids", 1, 2 ** 31 - 1)) == 1
    assert int(dump("ids", 1, 2 ** 31)) == 0
    assert int(dump("ids", 1, limit)) == 0
