"""The call sequences of tests/frame_sequences.py without a device.

1. Every committed sequence, as a script for the stand-alone slot-table program (csrc/vio_frame_slots.h with malloc for hipMalloc, built
   as in tests/test_frame_host_units.py; ASan and UBSan with VIO_TEST_SANITIZE=1), reaches what it is meant to reach: blocks handed from
   a frame to a frame of another geometry, from a mask to a frame and back, growth of the pool under full slots, a change of levels
   under resident frames, resets, a burst of pushes with nothing that waits between them.  These are conditions on the inputs of
   tests/test_gpu_frame_sequences.py, counted from the table the program prints; the counts are in DESIGN.md section 23.
2. run() over a stand-in made of the numpy restatements (StandInSequenceFrames of tests/test_frontend_frames.py): the driver runs, and
   its model's roll / reset / levels rules agree with that independent few-line implementation.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_reference as cr  # noqa: E402
import detect_reference as dr  # noqa: E402
import flow_reference as fr  # noqa: E402
import frame_sequences as fs  # noqa: E402
from test_frame_host_units import ALIGN, driver, layout, parse, run as run_program  # noqa: E402,F401
from test_frontend_frames import StandInSequenceFrames  # noqa: E402

SEEDS = [40, 56, 117]                   # the sequences of tests/test_gpu_frame_sequences.py: chosen here so that each meets REACH alone
N_OPS = 60
REACH = dict(frame_after_other_geometry=3, of_those_into_a_larger_block=1, frame_after_mask=1, mask_after_frame=1,
             growth_under_two_full_slots=1, levels_change_under_frames=1, resets=2, burst_after_single_push=1)


def mask_bytes(w, h):
    return ((w + 3) // 4 * 4 * h + ALIGN - 1) // ALIGN * ALIGN


def reach(script, lines):
    """What a script reached, counted from the tables the program printed after each of its lines."""
    c = dict.fromkeys(REACH, 0)
    levels, held, size, tab0, count0, single = 4, {}, {}, {}, 0, False
    for text, ln in zip(script, lines):
        letter, code, _, (_, count, _), tab = parse(ln)
        assert code == 0, (text, ln)                                   # FRAME_OK, and no allocator failure
        v = [int(x) for x in text.split()[1:]]
        full = sum(1 for s in tab0.values() if s[0] == 2)
        taken = []                                                      # (block, kind, w, h, bytes needed)
        if letter == "P":
            for k in range(v[0]):
                s, w, h = v[1 + 3 * k:4 + 3 * k]
                taken.append((tab[s][4], "frame", w, h, layout(w, h, levels)[1]))
            c["burst_after_single_push"] += 1 if single and v[0] >= 3 else 0
            single = v[0] == 1
        elif letter == "M":
            taken.append((tab[v[0]][5], "mask", v[1], v[2], mask_bytes(v[1], v[2])))
        elif letter == "R":
            c["resets"] += 1 if tab0.get(v[0], (0,))[0] > 0 else 0
        elif letter == "L":
            c["levels_change_under_frames"] += 1 if v[0] != levels and any(s[0] > 0 for s in tab0.values()) else 0
            levels = v[0]
        elif letter in "FTD":
            single = False                                              # (these wait for the device)
        c["growth_under_two_full_slots"] += 1 if count > count0 and full >= 2 else 0
        for blk, kind, w, h, need in taken:
            assert blk >= 0
            if blk not in held:
                assert blk >= count0
                size[blk] = need
            else:
                was = held[blk]
                assert need <= size[blk] <= 2 * need, (text, blk, size[blk], need)             # the pool's window
                if kind == "frame" and was[0] == "frame" and was[1:] != (w, h):
                    c["frame_after_other_geometry"] += 1
                    c["of_those_into_a_larger_block"] += 1 if size[blk] > need else 0
                c["frame_after_mask"] += 1 if kind == "frame" and was[0] == "mask" else 0
                c["mask_after_frame"] += 1 if kind == "mask" and was[0] == "frame" else 0
            held[blk] = (kind, w, h)
        tab0, count0 = tab, count
    return c


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_reaches_what_it_is_meant_to(driver, seed):  # noqa: F811
    seq = fs.make_sequence(seed, N_OPS)
    assert len(seq) == N_OPS and seq == fs.make_sequence(seed, N_OPS)                   # deterministic
    script = fs.to_slot_script(seq)
    lines = run_program(driver, script)
    got = reach(script, lines)
    print("seed %d: %s" % (seed, got))
    for k, least in REACH.items():
        assert got[k] >= least, (seed, k, got)
    # the program's table after each operation is the model's
    model, at = fs.Model(), 0
    for op in seq:
        one = fs.to_slot_script([op])
        at += len(one)
        if op[0] == "set_config":
            model.set_config(*op[1:])
        elif op[0] == "push":
            for (s, w, h, _, _) in op[1]:
                model.push(s, w, h, None)
        elif op[0] == "reset":
            model.reset(op[1])
        elif op[0] == "set_mask":
            model.set_mask(op[1], op[2], op[3], None)
        elif op[0] == "clear_mask":
            model.clear_mask(op[1])
        tab = parse(lines[at - 1])[4]
        want = {}
        for s in set(model.frames) | set(model.masks):
            w, h = model.shape.get(s, (0, 0))
            want[s] = (model.n_frames(s), w, h) + tuple(model.masks.get(s, (0, 0))[:2])
        assert {s: (t[0], t[1], t[2], t[6], t[7]) for s, t in tab.items()} == want, (op, tab, want)
    assert at == len(lines)


def test_both_flow_modes_among_the_seeds():
    assert {fs.make_sequence(s, 1)[0][4] for s in SEEDS} == {0, 1}


class NumpyOracle:
    """The numpy restatements behind the interface run() asks of an oracle."""

    def apply(self, img, clip_limit, tiles):
        return cr.apply(np.ascontiguousarray(img), clip_limit=clip_limit, tiles=tiles)

    def pyramid(self, level0, levels):
        return fr.pyramid(level0, levels)

    def track(self, prev0, next0, pts, guess, levels, half_patch, inverse):
        res = fr.multi_level(prev0, next0, pts, guess, levels=levels, half_patch=half_patch, inverse=inverse, order="wave64")
        return dict(zip(("next_pts", "status", "iterations", "cost"), res))

    def detect(self, img, tracked, track_cnt, mask, max_total, quality, min_distance):
        return dr.detect(img, tracked, track_cnt, mask, max_total, quality=quality, min_distance=min_distance)


def test_driver_over_the_stand_in():
    seq = fs.make_sequence(37, 15, shapes=[(17, 13), (32, 8)])
    kinds = [op[0] for op in seq]
    assert all(k in kinds for k in ("push", "track", "detect", "download", "reset")), kinds
    assert len({op[3] for op in seq if op[0] == "set_config"}) >= 2, "no change of levels"
    seen = fs.run(seq, StandInSequenceFrames(), NumpyOracle(), n_pts=4)
    assert len(seen) >= 8

    class Stuck(StandInSequenceFrames):
        """A wrong roll, which the driver must see: the slot's first frame stays prev for ever."""

        def push_batch(self, items):
            for it in items:
                old = self.slots.get(it.get("slot", 0), (None, None))
                StandInSequenceFrames.push_batch(self, [it])
                if old[0] is not None:
                    self.slots[it.get("slot", 0)] = (old[0], self.slots[it.get("slot", 0)][1])

    with pytest.raises(AssertionError):
        fs.run(seq, Stuck(), NumpyOracle(), n_pts=4)
