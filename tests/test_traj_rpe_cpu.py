"""The host half of the pose-error and association layer of splat_slam_amd.traj_eval: the declarations the binding is generated from,
argument validation, the TUM reader and writer, the command line's help and the pairing rule of the relative error.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from splat_slam_amd import _native as nat
from splat_slam_amd import traj_eval as te

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_both_entry_points_and_the_binding_exposes_them():
    hdr = open(os.path.join(ROOT, "include", "splat_hip.h")).read()
    for name, nargs in (("sgr_traj_associate", 13), ("sgr_traj_pose_errors", 20), ("sgr_traj_associate_scratch_bytes", 2),
                        ("sgr_traj_pose_errors_scratch_bytes", 1)):
        assert re.search(r"\b%s\(" % name, hdr), name
        assert len(nat.SIGNATURES[name][1]) == nargs, name
    assert nat.SIGNATURES["sgr_traj_associate_scratch_bytes"][0] is nat.C.c_size_t
    # sim3 is the one host pointer of sgr_traj_pose_errors; the index lists are device addresses
    args = nat.SIGNATURES["sgr_traj_pose_errors"][1]
    assert args[8] == nat.C.POINTER(nat.C.c_double) and args[5] is nat.C.c_void_p and args[6] is nat.C.c_void_p
    assert te.POSE_LAUNCHES == {"associate": nat.SGR_TRAJ_ASSOCIATE_LAUNCHES, "pose_errors": nat.SGR_TRAJ_POSE_ERRORS_LAUNCHES}
    assert all(1 <= v <= 4 for v in te.POSE_LAUNCHES.values())
    assert (nat.SGR_TRAJ_ABSOLUTE, nat.SGR_TRAJ_RELATIVE) == (0, 1) and nat.SGR_TRAJ_MAX_STAMPS == 2 ** 24
    assert te.RELATIONS == {"translation_part": nat.SGR_TRAJ_TRANSLATION_PART, "rotation_angle_rad": nat.SGR_TRAJ_ROTATION_ANGLE_RAD,
                            "rotation_angle_deg": nat.SGR_TRAJ_ROTATION_ANGLE_DEG, "rotation_part": nat.SGR_TRAJ_ROTATION_PART,
                            "full_transformation": nat.SGR_TRAJ_FULL_TRANSFORMATION}
    assert sorted(te.RELATIONS.values()) == [0, 1, 2, 3, 4]
    # what was there stays as it was
    assert te.LAUNCHES == {"accumulate": 2, "errors": 2} and nat.SGR_ABI_VERSION == 10


def test_arguments_are_validated_before_anything_touches_a_device():
    est, ref = torch.zeros(4, 7), np.tile(np.eye(4), (4, 1, 1))
    with pytest.raises(ValueError, match="relation"):
        te.pose_errors(est, ref, relation="translation")
    for delta in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="delta"):
            te.pose_errors(est, ref, delta=delta)
    with pytest.raises(ValueError, match="delta"):
        te.rpe(est, ref, delta=None)
    with pytest.raises(ValueError, match="indices"):
        te.pose_errors(est, ref, est_inds=torch.zeros(3, dtype=torch.int32), ref_inds=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        te.pose_errors(est, ref)
    with pytest.raises(RuntimeError, match="GPU"):
        te.ape_pose(est, ref, relation="rotation_part")
    with pytest.raises(RuntimeError, match="GPU"):
        te.associate(torch.zeros(3, dtype=torch.float64), np.zeros(3))
    with pytest.raises(ValueError, match="relation"):
        te.evaluate_files("no such file", "no such file", relation="angle")


def test_tum_files_round_trip_with_fp64_stamps_bit_for_bit(tmp_path):
    rng = np.random.default_rng(0)
    n = 50
    stamps = 1305031102.175304 + np.cumsum(rng.uniform(0.001, 0.1, n))             # TUM's epoch stamps: more digits than %.6f keeps
    stamps[3] = np.nextafter(stamps[2], np.inf)
    c2w = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        c2w[k, :3, :3] = q * np.sign(np.linalg.det(q))
    c2w[0, :3, :3] = np.diag([1.0, -1.0, -1.0])                                    # a half turn: w = 0
    c2w[1, :3, :3] = np.diag([-1.0, -1.0, 1.0])
    c2w[:, :3, 3] = rng.normal(size=(n, 3)) * 10.0
    path = tmp_path / "sub" / "traj.txt"
    te.write_tum_trajectory(path, stamps, c2w)
    got_stamps, got = te.read_tum_trajectory(path)
    assert got_stamps.dtype == np.float64 and got_stamps.tobytes() == stamps.tobytes()
    assert np.array_equal(got[:, :3, 3], c2w[:, :3, 3]) and np.abs(got - c2w).max() < 1e-14
    # a second trip gives the same file: comment lines, empty lines and torch input
    with open(path) as fp:
        text = fp.read()
    with open(path, "w") as fp:
        fp.write("# a comment\n\n" + text.replace("\n", "   # trailing\n", 1))
    again_stamps, again = te.read_tum_trajectory(path)
    assert again_stamps.tobytes() == stamps.tobytes() and np.array_equal(again, got)
    te.write_tum_trajectory(tmp_path / "b.txt", torch.from_numpy(stamps), torch.from_numpy(got))
    assert np.array_equal(te.read_tum_trajectory(tmp_path / "b.txt")[0], stamps)
    with open(path, "a") as fp:
        fp.write("1.0 2.0 3.0\n")
    with pytest.raises(ValueError, match="fields"):
        te.read_tum_trajectory(path)
    with pytest.raises(ValueError):
        te.write_tum_trajectory(path, stamps[:3], c2w)


def test_the_command_lines_help_exits_0(capsys):
    with pytest.raises(SystemExit) as e:
        te.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--max-diff", "--offset", "--no-scale", "--rpe-delta", "--all-pairs", "--relation", "--out"):
        assert flag in text


def restated_pairs(c, delta, all_pairs):
    """the rule in plain words: all_pairs pairs every used pose with the one delta further on; otherwise the walk starts at pose 0 and
    hops by delta, and every hop that lands inside the trajectory is a pair"""
    pairs = []
    if all_pairs:
        for r in range(c):
            if r + delta <= c - 1:
                pairs.append((r, r + delta))
        return pairs
    at = 0
    while at + delta <= c - 1:
        pairs.append((at, at + delta))
        at += delta
    return pairs


def test_pair_enumeration():
    assert te.item_pairs(7, 3, False) == [(0, 3), (3, 6)]
    assert te.item_pairs(7, 3, True) == [(0, 3), (1, 4), (2, 5), (3, 6)]
    assert te.item_pairs(6, 3, False) == [(0, 3)] and te.item_pairs(4, 3, True) == [(0, 3)]
    assert te.item_pairs(5, 1, False) == te.item_pairs(5, 1, True) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    for delta in (1, 2, 3, 7):
        for c in (0, 1, delta, delta + 1, 2 * delta, 2 * delta + 1):
            for all_pairs in (False, True):
                got = te.item_pairs(c, delta, all_pairs)
                assert got == restated_pairs(c, delta, all_pairs), (c, delta, all_pairs)
                assert len(got) == (max(c - delta, 0) if all_pairs else (c - 1) // delta if c else 0)
    assert te.item_pairs(3, 3, False) == te.item_pairs(3, 3, True) == te.item_pairs(0, 1, True) == []
    with pytest.raises(ValueError):
        te.item_pairs(5, 0, False)


def test_the_keys_of_the_extra_results():
    assert te.extra_key("translation_part", 5, False) == "rpe_translation_part_d5"
    assert te.extra_key("rotation_part", 2, True) == "rpe_rotation_part_d2_all"
    assert te.extra_key("rotation_angle_deg", None, False) == "ape_rotation_angle_deg"
