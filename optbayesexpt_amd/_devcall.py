"""The mechanics around a tiled library call that the feature modules share: device addresses, the cloud of an
experiment object, a workspace per call and the tiles of a request.  Plain functions; the argument lists of the entry
points stay with their callers."""
import ctypes

import torch

P = ctypes.c_void_p


def ptr(t):
    return P(t.data_ptr())


def cloud(obe):
    """Device ``(particles, weights)`` of ``obe._parameters``; host edits of the cloud are uploaded here."""
    p, w = obe._parameters.tensor(), obe._weights.tensor()
    if p.shape[1] != w.shape[0]:
        raise ValueError("particles and particle_weights have different lengths")
    return p, w


def workspace(lib, device, query, *sizes):
    """``(tensor, nbytes)`` of what ``lib``'s ``query(*sizes)`` asks for.  A workspace of the call's own (torch's caching
    allocator hands the same block back call after call): the object's workspace keeps the record of a sweep enqueued
    ahead, which must stay readable."""
    nbytes = int(getattr(lib.cdll, query)(*sizes))
    return torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=device), nbytes


def model_call(obe, entry, query, sizes, *args):
    """``entry`` of the object's model library on ``args``, then a workspace of ``query(*sizes)`` bytes and the
    stream: what every model-dependent entry point ends in."""
    ws, nbytes = workspace(obe._mlib, obe._device, query, *sizes)
    obe._mlib.call(entry, obe._model_struct, *args, ptr(ws), nbytes, obe._stream())


def column_tiles(x, per_call):
    """Contiguous (rows, <= per_call) pieces of the columns of ``x`` with their first column."""
    n_x = x.shape[1]
    if n_x <= per_call:
        yield 0, x
        return
    for start in range(0, n_x, per_call):
        yield start, x[:, start:start + per_call].contiguous()
