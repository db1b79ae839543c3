"""Frame batches of a scene, loaded one batch ahead of the GPU: the loader of Map.create_explored_map, Map.audit_visibility and
GTMap.create_map."""
from __future__ import annotations

import queue
import threading

import numpy as np

from ..utils.mapping_utils import load_depth_npy


def depth_batch(paths, lo, hi) -> np.ndarray:
    """(hi - lo, H, W) float32 metres: the depth frames paths[lo:hi]"""
    return np.stack([np.asarray(load_depth_npy(paths[i]), dtype=np.float32) for i in range(lo, hi)])


def batch_ranges(n, batch):
    """(lo, hi) of n frames in batches of `batch`"""
    return [(lo, min(n, lo + int(batch))) for lo in range(0, n, int(batch))]


def prefetch(load, ranges, name):
    """-> a generator of load(*r) for every r of `ranges` -- (lo, hi), or (directory, lo, hi) for a walk over several -- in order.
    load runs on a daemon thread called `name`, which starts with this call and stays ahead of the consumer by a two-slot queue; an
    exception of load is raised from the generator, on the consuming thread; the thread is joined when the last item has been
    taken."""
    items = queue.Queue(maxsize=2)

    def work():
        try:
            for r in ranges:
                items.put(load(*r))
            items.put(None)
        except BaseException as e:          # surfaced on the calling thread
            items.put(e)
    loader = threading.Thread(target=work, name=name, daemon=True)
    loader.start()

    def take():
        while True:
            item = items.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            yield item
        loader.join()
    return take()
