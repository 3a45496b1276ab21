"""Chunk coalescer: fills every launch with ``max_batch`` 4 s chunks taken across loader items.

The reference's unit of use is ``Tester_Enhance.inference(data_loader, saveDir)`` over a loader with ``batch_size: 1``
(tester.py:846-975, config/NN_BSS.yml:108-111): one item is one recording, cut into 1-3 splits.  Run item by item, a
launch holds the splits of ONE item (B = 1-3); the fused pipeline is at its best at B = 16.  Results do not depend on the
batch an utterance runs in, bit for bit, so the chunks of consecutive items can share launches.

This module is the planning half, with no GPU dependency: it reads items, cuts them into chunks tagged
``(item, b, split)``, hands batches of exactly ``max_batch`` chunks to a runner (the remainder at the end of the loader as
one short batch; a change of the items' shape key -- the frame count T -- flushes early, since a launch has one T), keeps
at most ``depth`` batches in flight, and hands completed items out in loader order.  The runner is two callables:

    submit(index, chunks) -> handle      enqueue batch ``index`` (asynchronous); ``chunks`` is a list of ``Chunk``
    collect(handle) -> rows              wait for that batch; one output per chunk, in the batch's row order

``collect`` is called on the oldest batch in flight only, before a new ``submit`` when ``depth`` batches are in flight
and at the end.  The loader is read ahead by at most one item past ``max_batch`` pending chunks.
"""
from __future__ import annotations

import collections
from typing import Any, Callable, Hashable, Iterable, Iterator, List, NamedTuple, Optional


class Item:
    """One loader item: ``n_b`` utterances (the loader's batch) x ``n_split`` chunks each, all of shape key ``key``.
    ``payload`` is the caller's (the loader tuple, a recording); ``outputs[split][b]`` is filled as batches complete."""
    __slots__ = ("index", "n_b", "n_split", "key", "payload", "outputs", "missing")

    def __init__(self, index: int, n_b: int, n_split: int, key: Hashable, payload: Any = None):
        if n_b < 1 or n_split < 1:
            raise ValueError(f"an item needs at least one utterance and one split, got B = {n_b}, splits = {n_split}")
        self.index, self.n_b, self.n_split, self.key, self.payload = index, int(n_b), int(n_split), key, payload
        self.outputs: List[List[Any]] = [[None] * self.n_b for _ in range(self.n_split)]
        self.missing = self.n_b * self.n_split


class Chunk(NamedTuple):
    item: Item
    b: int
    split: int


def coalesce(items: Iterable[Item], submit: Callable[[int, List[Chunk]], Any], collect: Callable[[Any], List[Any]],
             max_batch: int, depth: int = 2) -> Iterator[Item]:
    """Run the chunks of ``items`` in batches of ``max_batch`` through ``submit`` / ``collect``; yield every item, in
    loader order, once all its chunks' outputs are in ``item.outputs``.  Chunks are queued item by item, within an item
    split-major (split 0 of every utterance, then split 1, ...: the row order of the item-by-item schedule)."""
    max_batch, depth = int(max_batch), max(1, int(depth))
    if max_batch < 1:
        raise ValueError(f"max_batch must be >= 1, got {max_batch}")
    queue: collections.deque = collections.deque()          # chunks read but not yet submitted
    in_flight: collections.deque = collections.deque()      # (handle, chunks) in submission order
    waiting: collections.deque = collections.deque()        # items read, not yet handed out (loader order)
    n_batches = 0

    def retire():
        handle, chunks = in_flight.popleft()
        rows = collect(handle)
        if len(rows) != len(chunks):
            raise RuntimeError(f"runner returned {len(rows)} rows for a batch of {len(chunks)} chunks")
        for c, r in zip(chunks, rows):
            c.item.outputs[c.split][c.b] = r
            c.item.missing -= 1

    def launch(n):
        nonlocal n_batches
        while len(in_flight) >= depth:
            retire()
        chunks = [queue.popleft() for _ in range(n)]
        in_flight.append((submit(n_batches, chunks), chunks))
        n_batches += 1

    def ready():
        while waiting and waiting[0].missing == 0:
            yield waiting.popleft()

    key: Optional[Hashable] = None
    for it in items:
        if queue and it.key != key:                          # a launch has one shape: flush the short batch
            launch(len(queue))
            yield from ready()
        key = it.key
        waiting.append(it)
        queue.extend(Chunk(it, b, k) for k in range(it.n_split) for b in range(it.n_b))
        while len(queue) >= max_batch:
            launch(max_batch)
            yield from ready()
    if queue:
        launch(len(queue))
    while in_flight:
        retire()
        yield from ready()
    if waiting:                                              # (cannot happen: every chunk was submitted and collected)
        raise RuntimeError("coalesce: items left incomplete")
