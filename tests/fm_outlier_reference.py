"""What include/vio_fm_outlier.h's vio_fm_remove_batch is held to, over tests/fm_reference.py's track lists: the erase loop behind
removeOutlier's `return;` (feature_manager.cpp:259-275), which is removeFailures' (:161-171) keyed on another field, with the rows
named by feature id; and NumpyFmOutlier, fm_stream_reference.NumpyFm with that call, so that a StreamDriver(features=(NumpyFmOutlier,
slot), outlier_px=x) runs without a device."""
import numpy as np

import fm_reference as fr
import fm_stream_reference as fsr


def remove_ids(tracks, ids):
    """(the tracks whose id is not listed, in their order and untouched; erased (len(ids),) bool: which ids named a track)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if len(np.unique(ids)) != len(ids):
        raise ValueError("an id is listed twice")
    have = {int(t["id"]) for t in tracks}
    gone = {int(i) for i in ids}
    return [t for t in fr.copy_tracks(tracks) if t["id"] not in gone], np.array([int(i) in have for i in ids], dtype=bool)


class NumpyFmOutlier(fsr.NumpyFm):
    def remove_batch(self, items):
        self._slots_once("remove_batch", [it[0] for it in items])
        out = []
        for slot, ids in items:
            ids = np.asarray(ids, dtype=np.int64)
            if ids.ndim != 1 or len(ids) > fr.MAX_TRACKS:
                raise ValueError("ids: one dimension, at most %d" % fr.MAX_TRACKS)
            new, erased = remove_ids(self.slots.setdefault(int(slot), []), ids)
            self.slots[int(slot)] = new
            out.append(self._res(slot, n_rows=int(erased.sum()), erased=erased))
        return out
