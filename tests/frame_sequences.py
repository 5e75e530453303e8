"""A model-based driver for sequences of calls on the resident-frame library (include/vio_frame.h).  No tests in here:
tests/test_frame_sequences_cpu.py runs it over a stand-in and through the stand-alone slot-table program, tests/test_gpu_frame_sequences.py
over frame.FrameHandle and the three host-array handles.

    make_sequence(seed, n_ops)            a deterministic list of legal operations over SLOTS slots (tuples, see below)
    Model                                 the shadow state with the header's rules: the roll, reset keeps the mask, a change of levels drops
                                          every frame and keeps every mask, level 0 is fixed at push time by the settings of that moment
    run(sequence, frames, oracle)         applies every operation to `frames` and to the model and holds whatever `frames` returns to the
                                          model through `oracle`, byte for byte; sweeps every resident level at the end
    to_slot_script(sequence)              the same sequence in tests/cpp/frame_slots_main.cpp's input language

Operations:
    ("set_config", equalize, tiles, levels, inverse)
    ("push", ((slot, w, h, seed, t), ...))      image(w, h, seed, t) into each slot, one push_batch
    ("reset", slot)
    ("set_mask", slot, w, h, kind)              mask_image(w, h, kind)          ("clear_mask", slot)
    ("track", slots, with_guess)                one track_batch over every slot with two frames
    ("detect", slots)                           one detect_batch over every slot with a frame and no mask of another geometry
    ("download", slot, which, level)

`oracle` has
    apply(img, clip_limit, tiles)                                  level 0 of an equalised push
    pyramid(level0, levels)                                        the list of levels
    track(prev0, next0, pts, guess, levels, half_patch, inverse)   FlowHandle.track's dict
    detect(img, tracked, track_cnt, mask, max_total, quality, min_distance)    DetectHandle.detect's dict
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_reference as flow_ref  # noqa: E402
from test_gpu_frame import detect_bytes, points, same_bytes, same_detect, same_track, track_bytes  # noqa: E402

PREV, NEXT = 0, 1
SLOTS = 4
# block sizes at 2 levels: 3840, 3840, 2816, 768, 768, 512 bytes: inside and outside the pool's window of twice the request
SHAPES = [(64, 48), (61, 45), (129, 17), (33, 9), (17, 13), (32, 8)]
TILES = [(8, 8), (3, 5), (16, 16)]
LEVELS = [1, 2, 3]
SHIFT = (1.3, -0.7)
CLIP_LIMIT, HALF_PATCH, QUALITY, MIN_DISTANCE, MAX_TOTAL, N_TRACKED = 3.0, 2, 0.01, 3, 40, 9
_cache = {}


def legal(w, h, levels):
    """Every one of the levels is at least 2 x 2."""
    return (w >> (levels - 1)) >= 2 and (h >> (levels - 1)) >= 2


def image(w, h, seed, t):
    """Frame t of a stream: one texture sampled t small shifts further, so that points track from a frame into the next.  Every third
    frame has rows of another stride than its width, the bytes between them 255."""
    key = ("image", w, h, seed, t)
    if key not in _cache:
        img = flow_ref.texture(w, h, seed=seed, shift=(SHIFT[0] * t, SHIFT[1] * t), smooth=1.5)
        if t % 3 == 2:
            wide = np.full((h, w + 5), 255, dtype=np.uint8)
            wide[:, :w] = img
            img = wide[:, :w]
        _cache[key] = img
    return _cache[key]


def mask_image(w, h, kind):
    """0: the left third closed; 1: a closed row and a closed column, strided rows whose padding is 255; 2: closed 4 x 4 squares."""
    key = ("mask", w, h, kind)
    if key not in _cache:
        m = np.full((h, w + 3), 255, dtype=np.uint8)
        if kind == 0:
            m[:, : w // 3] = 0
        elif kind == 1:
            m[h // 2, :w] = 0
            m[:, w // 2] = 0
        else:
            yy, xx = np.mgrid[0:h, 0:w + 3]
            m[((yy // 4) + (xx // 4)) % 3 == 0] = 0
            m[:, w:] = 255
        _cache[key] = m[:, :w] if kind == 1 else np.ascontiguousarray(m[:, :w])
    return _cache[key]


class Model:
    """What the handle must hold.  Level 0 of a frame is whatever the caller hands to push (an array in run(), None in make_sequence,
    which needs the occupancy alone)."""

    def __init__(self):
        self.equalize, self.tiles, self.levels, self.inverse = False, (8, 8), 4, 0      # a new handle's settings
        self.frames = {}            # slot -> [level 0 of prev, level 0 of next] or [level 0 of next]
        self.shape = {}             # slot -> (w, h) of its frames
        self.masks = {}             # slot -> (w, h, array or None)

    def set_config(self, equalize, tiles, levels, inverse):
        if levels != self.levels:                       # every frame goes, every mask stays
            self.frames, self.shape = {}, {}
        self.equalize, self.tiles, self.levels, self.inverse = bool(equalize), tuple(tiles), int(levels), int(inverse)

    def push(self, slot, w, h, level0):
        assert self.shape.get(slot, (w, h)) == (w, h) and legal(w, h, self.levels), (slot, w, h)
        self.shape[slot] = (w, h)
        self.frames[slot] = (self.frames.get(slot, []) + [level0])[-2:]

    def reset(self, slot):
        self.frames.pop(slot, None)
        self.shape.pop(slot, None)

    def set_mask(self, slot, w, h, mask):
        self.masks[slot] = (w, h, mask)

    def clear_mask(self, slot):
        self.masks.pop(slot, None)

    def n_frames(self, slot):
        return len(self.frames.get(slot, []))

    def frame(self, slot, which):
        f = self.frames[slot]
        assert len(f) == 2 or which == NEXT
        return f[-1] if which == NEXT else f[0]

    def trackable(self):
        return tuple(s for s in sorted(self.frames) if len(self.frames[s]) == 2)

    def detectable(self):
        return tuple(s for s in sorted(self.frames) if s not in self.masks or self.masks[s][:2] == self.shape[s])

    def mask(self, slot):
        return self.masks[slot][2] if slot in self.masks else None


def make_sequence(seed, n_ops, inverse=None, shapes=SHAPES):
    """n_ops legal operations, the first a set_config; inverse: the flow mode of the whole sequence (default: the seed's parity)."""
    rng = np.random.RandomState(seed)
    inverse = int(seed) & 1 if inverse is None else int(inverse)
    m = Model()
    t_of = {}                                           # slot -> (stream seed, frames pushed so far)
    n_streams = 0
    kinds = ["push", "track", "detect", "download", "reset", "set_mask", "clear_mask", "set_config"]
    weights = np.array([0.38, 0.10, 0.10, 0.10, 0.09, 0.09, 0.04, 0.10])
    ops = [("set_config", bool(rng.randint(2)), TILES[rng.randint(3)], 2, inverse)]
    m.set_config(*ops[0][1:])
    while len(ops) < n_ops:
        kind = kinds[rng.choice(len(kinds), p=weights)]
        if kind == "push":
            slots = sorted(rng.choice(SLOTS, size=rng.randint(1, SLOTS + 1), replace=False).tolist())
            items = []
            for s in slots:
                if s in m.shape:
                    w, h = m.shape[s]
                else:
                    ok = [sh for sh in shapes if legal(sh[0], sh[1], m.levels)]
                    w, h = ok[rng.randint(len(ok))]
                    if s in m.masks and legal(m.masks[s][0], m.masks[s][1], m.levels) and rng.uniform() < 0.7:
                        w, h = m.masks[s][:2]
                    n_streams += 1
                    t_of[s] = (100 * seed + n_streams, 0)
                stream, t = t_of[s]
                items.append((s, w, h, stream, t))
                t_of[s] = (stream, t + 1)
                m.push(s, w, h, None)
            ops.append(("push", tuple(items)))
        elif kind == "track":
            if m.trackable():
                ops.append(("track", m.trackable(), bool(rng.randint(2))))
        elif kind == "detect":
            if m.detectable():
                ops.append(("detect", m.detectable()))
        elif kind == "download":
            if m.frames:
                s = sorted(m.frames)[rng.randint(len(m.frames))]
                which = NEXT if m.n_frames(s) < 2 else int(rng.randint(2))
                ops.append(("download", s, which, int(rng.randint(m.levels))))
        elif kind == "reset":
            if m.frames:
                s = sorted(m.frames)[rng.randint(len(m.frames))]
                m.reset(s)
                ops.append(("reset", s))
        elif kind == "set_mask":
            s = int(rng.randint(SLOTS))
            w, h = m.shape[s] if s in m.shape and rng.uniform() < 0.85 else shapes[rng.randint(len(shapes))]
            m.set_mask(s, w, h, None)
            ops.append(("set_mask", s, w, h, int(rng.randint(3))))
        elif kind == "clear_mask":
            if m.masks:
                s = sorted(m.masks)[rng.randint(len(m.masks))]
                m.clear_mask(s)
                ops.append(("clear_mask", s))
        else:
            equalize, tiles, levels = m.equalize, m.tiles, m.levels
            what = rng.randint(3)
            if what == 0:
                equalize = not equalize
            elif what == 1:
                tiles = [t for t in TILES if t != tiles][rng.randint(2)]
            else:
                levels = [n for n in LEVELS if n != levels][rng.randint(2)]
            m.set_config(equalize, tiles, levels, inverse)
            ops.append(("set_config", equalize, tiles, levels, inverse))
    return ops


def to_slot_script(sequence):
    """The sequence as lines for tests/cpp/frame_slots_main.cpp (a track or detect over several slots is a line per slot)."""
    out = []
    for op in sequence:
        if op[0] == "push":
            out.append("P %d " % len(op[1]) + " ".join("%d %d %d" % it[:3] for it in op[1]))
        elif op[0] == "reset":
            out.append("R %d" % op[1])
        elif op[0] == "set_config":
            out.append("L %d" % op[3])
        elif op[0] == "set_mask":
            out.append("M %d %d %d" % op[1:4])
        elif op[0] == "clear_mask":
            out.append("C %d" % op[1])
        elif op[0] == "track":
            out += ["T %d" % s for s in op[1]]
        elif op[0] == "detect":
            out += ["D %d" % s for s in op[1]]
        else:
            assert op[0] == "download", op
            out.append("F %d %d %d" % op[1:4])
    return out


def configure(frames, model):
    frames.set_config(equalize=model.equalize, clahe=dict(clip_limit=CLIP_LIMIT, tiles=model.tiles),
                      flow=dict(levels=model.levels, half_patch=HALF_PATCH, inverse=model.inverse),
                      detect=dict(quality=QUALITY, min_distance=MIN_DISTANCE))


def check_download(frames, oracle, model, slot, which, level, name, seen):
    got = frames.download(slot, which, level)
    same_bytes(got, oracle.pyramid(model.frame(slot, which), model.levels)[level], name)
    seen.append((name, got.tobytes()))


def check_track(frames, oracle, model, slots, with_guess, n_pts, name, seen):
    assert tuple(slots) == model.trackable(), (name, slots, model.trackable())
    items = []
    for s in slots:
        pts = points(*model.shape[s], n=n_pts)
        items.append(dict(slot=s, prev_pts=pts, guess=(pts + np.float32(0.5)).astype(np.float32) if with_guess else None))
    outs = frames.track_batch(items)
    assert len(outs) == len(slots)
    for s, it, got in zip(slots, items, outs):
        ref = oracle.track(model.frame(s, PREV), model.frame(s, NEXT), it["prev_pts"], it["guess"], model.levels, HALF_PATCH, model.inverse)
        same_track(got, ref, (name, "slot", s))
        seen.append(((name, s), track_bytes(got)))


def check_detect(frames, oracle, model, slots, name, seen):
    assert tuple(slots) == model.detectable(), (name, slots, model.detectable())
    items = []
    for s in slots:
        w, h = model.shape[s]
        items.append(dict(slot=s, tracked=points(w, h)[:N_TRACKED], track_cnt=np.arange(N_TRACKED, dtype=np.int32) % 3 + 1, max_total=MAX_TOTAL))
    outs = frames.detect_batch(items)
    assert len(outs) == len(slots)
    for s, it, got in zip(slots, items, outs):
        mask = model.mask(s)
        ref = oracle.detect(model.frame(s, NEXT), it["tracked"], it["track_cnt"], None if mask is None else np.ascontiguousarray(mask),
                            MAX_TOTAL, QUALITY, MIN_DISTANCE)
        same_detect(got, ref, (name, "slot", s))
        seen.append(((name, s), detect_bytes(got)))


def run(sequence, frames, oracle, n_pts=70):
    """Every operation on `frames` and on the model; every result `frames` returns against the model's through `oracle`; at the end
    every level of every resident frame, one track_batch and one detect_batch.  Returns [(name, bytes)] of all that was compared."""
    model, seen = Model(), []
    for i, op in enumerate(sequence):
        name = (i,) + tuple(op[:1])
        if op[0] == "set_config":
            model.set_config(*op[1:])
            configure(frames, model)
        elif op[0] == "push":
            imgs = [image(w, h, seed, t) for (_, w, h, seed, t) in op[1]]
            frames.push_batch([dict(slot=it[0], img=img) for it, img in zip(op[1], imgs)])
            for (s, w, h, _, _), img in zip(op[1], imgs):
                model.push(s, w, h, oracle.apply(img, CLIP_LIMIT, model.tiles) if model.equalize else np.ascontiguousarray(img))
        elif op[0] == "reset":
            frames.reset(op[1])
            model.reset(op[1])
        elif op[0] == "set_mask":
            mask = mask_image(*op[2:5])
            frames.set_mask(mask, slot=op[1])
            model.set_mask(op[1], op[2], op[3], mask)
        elif op[0] == "clear_mask":
            frames.set_mask(None, slot=op[1])
            model.clear_mask(op[1])
        elif op[0] == "track":
            check_track(frames, oracle, model, op[1], op[2], n_pts, name, seen)
        elif op[0] == "detect":
            check_detect(frames, oracle, model, op[1], name, seen)
        else:
            assert op[0] == "download", op
            check_download(frames, oracle, model, op[1], op[2], op[3], name + tuple(op[1:]), seen)
    for s in sorted(model.frames):
        for which in ((PREV, NEXT) if model.n_frames(s) == 2 else (NEXT,)):
            for l in range(model.levels):
                check_download(frames, oracle, model, s, which, l, ("sweep", s, which, l), seen)
    if model.trackable():
        check_track(frames, oracle, model, model.trackable(), False, n_pts, ("sweep", "track"), seen)
    if model.detectable():
        check_detect(frames, oracle, model, model.detectable(), ("sweep", "detect"), seen)
    return seen
