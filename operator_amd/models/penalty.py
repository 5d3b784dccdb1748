"""Per-request token table for the repetition / frequency / presence penalties
(docs/PARITY.md "Sampling: penalties"; csrc/kernels/penalty.hip).

A penalised request owns one slot from admission until it is reaped. Per slot:

* ``cnt`` int32 [slots, vocab]: bit 31 = the token occurs in the prompt, bits 0-30 = how
  often it was generated;
* ``lst`` int32 [slots, cap]: the distinct tokens whose ``cnt`` word is non-zero, in any
  order, so a decode step touches a row's ~1k seen tokens and not its vocabulary, and a
  slot is cleared by walking its previous occupant's list instead of a vocab-wide memset;
* ``n`` int32 [slots]: the length of that list.

The tensors are written on the device only (``ops.penalty_seed`` at prefill, ``ops.sample_penalty``
inside every decode step); the free list of slots is host-side. A slot handed back is not
cleared: its next seeding does that, after the previous occupant's last kernel in stream order.
"""
from __future__ import annotations

import torch


class PenaltyTable:
    def __init__(self, slots: int, vocab: int, cap: int, device: str | torch.device = "cuda"):
        if slots < 1 or vocab < 1 or cap < 1:
            raise ValueError("penalty table: slots, vocab and cap must be positive")
        self.slots, self.vocab, self.cap = slots, vocab, cap
        self.cnt = torch.zeros(slots, vocab, dtype=torch.int32, device=device)
        self.lst = torch.zeros(slots, cap, dtype=torch.int32, device=device)
        self.n = torch.zeros(slots, dtype=torch.int32, device=device)
        self._free = list(range(slots - 1, -1, -1))

    @property
    def free(self) -> int:
        return len(self._free)

    def take(self) -> int:
        """A free slot (the most recently returned one first), -1 when none is left."""
        return self._free.pop() if self._free else -1

    def give(self, slot: int) -> None:
        if slot >= 0:
            self._free.append(slot)
