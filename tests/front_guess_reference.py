"""A numpy restatement of the prediction's rule in the front end, written from frontend.FeatureTracker's lines
(_take_guess and read_image's fallback) and from nothing under test.  No tests in here.

    take_guess(cur, ids, pred_ids, pred_px)      (guess (n, 2) float32, hit (n,) bool): the predicted pixel for a point whose id is
                                                 listed (of a repeated id the first listed row), the point's own pixel otherwise
    normalise(pred_ids, pred_px)                 the rows as they go to the device: ids ascending, the first listed row of each id
    find(sorted_ids, ids)                        per id its row among sorted_ids, -1 where it is not there or is negative
    falls_back(guessed, n_ok, min_tracked)       read_image's condition for the second call
"""
import numpy as np


def take_guess(cur, ids, pred_ids, pred_px):
    pred_ids = np.asarray(pred_ids, dtype=np.int64).reshape(-1)
    pred_px = np.asarray(pred_px, dtype=np.float32).reshape(-1, 2)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    guess = np.array(cur, dtype=np.float32).reshape(-1, 2)
    order = np.argsort(pred_ids, kind="stable")
    at = np.searchsorted(pred_ids[order], ids)
    hit = (at < len(order)) & (ids >= 0)
    hit[hit] = pred_ids[order][at[hit]] == ids[hit]
    guess[hit] = pred_px[order][at[hit]]
    return guess, hit


def normalise(pred_ids, pred_px):
    pred_ids = np.asarray(pred_ids, dtype=np.int64).reshape(-1)
    pred_px = np.asarray(pred_px, dtype=np.float32).reshape(-1, 2)
    order = np.argsort(pred_ids, kind="stable")
    s = pred_ids[order]
    first = np.ones(len(s), dtype=bool)
    first[1:] = s[1:] != s[:-1]
    return s[first].copy(), pred_px[order][first].copy()


def find(sorted_ids, ids):
    sorted_ids = np.asarray(sorted_ids, dtype=np.int64).reshape(-1)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    at = np.searchsorted(sorted_ids, ids)
    hit = (at < len(sorted_ids)) & (ids >= 0)
    hit[hit] = sorted_ids[at[hit]] == ids[hit]
    return np.where(hit, at, -1).astype(np.int32)


def falls_back(guessed, n_ok, min_tracked):
    """read_image: `guess is not None and self.min_tracked is not None and n_ok < self.min_tracked`; min_tracked 0 stands for None."""
    return bool(guessed) and int(n_ok) < int(min_tracked)
