"""Reads from either strand.  A sequencer reads a molecule from whichever end it meets: about half of all real reads are the
reverse complement of what the template shows.  rc(r)[x] = comp(r[L-1-x]) with a<->t, c<->g and the letter's case kept; every
other byte stays where the reversal puts it.  Plain Python, no GPU: the device never sees a turned read (a job carries its
strand, include/pia.h and include/prc.h), this is what the host side and the tests turn reads with."""
import random

_COMP = bytes.maketrans(b"acgtACGT", b"tgcaTGCA")


def reverse_complement(seq: bytes) -> bytes:
    return bytes(seq).translate(_COMP)[::-1]


def seeded_mask(n: int, seed: int):
    """n strands as a sequencer would deal them, each 1 (reverse) with probability one half, from random.Random(seed)"""
    rng = random.Random(seed)
    return [rng.randrange(2) for _ in range(n)]


def turn(reads, mask):
    """reads[j] where mask[j] is 0, its reverse complement where it is 1"""
    return [reverse_complement(r) if m else bytes(r) for r, m in zip(reads, mask)]
