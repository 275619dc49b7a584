"""Canonical 31-mers built from chosen hash values, for the tests of what classify derives from ku_fmix64(canonical k-mer).

The hash of the HyperLogLog sketches (murmurhash3's finalizer of value + 1, hyperloglogplus.cpp:830-838) is a bijection of the
64-bit values, so a hash with any bits prescribed has preimages: unmix(h).  A k-mer of classify is more than a value -- it
is below 4^k and not above its reverse complement -- which about one value in eight is for k = 31, so build() draws the bits
left free until the preimage is one.  Where few bits are free the hashes are few: rank 53 of the dense sketch (p = 12) and
add = 40 of a flagged sparse encoding (p' = 25) leave none -- ONE hash per register index, 500 of the 4096 with a canonical
31-mer behind them (register 7 has one; 0 and 4095 have none, unmix(0) is 2^64 - 1) -- and rank 52 / add = 39 likewise.  build()
then goes through all of them and raises NoKmer when none fits; first_dense() and first_flagged() walk on to the next index
that has one.

The bits of a hash h, from the top: 12 bits register index (p = 12), behind them the dense rank = leading zeros + 1 (53: none
set); 25 bits sparse index (p' = 25) -- an encoding is "flagged" when the 13 behind the register index are zero, and then carries
add = leading zeros behind the 25 + 1 (40: none set), the dense rank being 13 + add."""
import numpy as np

M64 = (1 << 64) - 1
K = 31
_ENUMERATE_BELOW = 12  # free bits: fewer than this and build() tries every hash, in a drawn order
_TRIES = 4096  # draws otherwise: about one in eight fits, so (7/8)^4096 to fail
_DEFAULT_RNG = np.random.default_rng(31)  # of the builders called without one


class NoKmer(LookupError):
    """no canonical k-mer has a hash with the prescribed bits"""


def unmix(h):
    """the value whose hash (murmurhash3_finalizer of value + 1) is h: both multipliers are odd, x ^= x >> 33 undoes itself"""
    x = h
    x ^= x >> 33
    x = x * pow(0xc4ceb9fe1a85ec53, -1, 1 << 64) & M64
    x ^= x >> 33
    x = x * pow(0xff51afd7ed558ccd, -1, 1 << 64) & M64
    x ^= x >> 33
    return (x - 1) & M64


def revcomp(v, k=K):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (v & 3))
        v >>= 2
    return r


def is_canonical_kmer(v, k=K):
    return v < 4 ** k and v <= revcomp(v, k)


def build(fixed_mask, fixed_val, rng, k=K):
    """(h, v): h & fixed_mask == fixed_val & fixed_mask, the other bits drawn from rng (a numpy Generator), v = unmix(h) a
    canonical k-mer; NoKmer when there is none"""
    fixed_val &= fixed_mask
    free = [b for b in range(64) if not (fixed_mask >> b) & 1]
    if len(free) < _ENUMERATE_BELOW:
        for x in rng.permutation(1 << len(free)).tolist():
            h = fixed_val
            for j, b in enumerate(free):
                h |= ((x >> j) & 1) << b
            v = unmix(h)
            if is_canonical_kmer(v, k):
                return h, v
        raise NoKmer(f"none of the {1 << len(free)} hashes {fixed_val:#018x} / {fixed_mask:#018x} is a canonical {k}-mer's")
    for _ in range(_TRIES):
        h = fixed_val | (int(rng.integers(0, 1 << 64, dtype=np.uint64)) & ~fixed_mask & M64)
        v = unmix(h)
        if is_canonical_kmer(v, k):
            return h, v
    raise NoKmer(f"{_TRIES} draws")


def _top(bits):
    return ((1 << bits) - 1) << (64 - bits)


def dense(idx, rank, rng=None):
    """register idx (0..4095) of the dense sketch gets exactly `rank` (1..53; 53: no bit set behind the index)"""
    assert 0 <= idx < 4096 and 1 <= rank <= 53
    bits = min(12 + rank, 64)  # the index, rank - 1 zeros, a one
    return build(_top(bits), (idx << 52) | ((1 << (52 - rank)) if rank < 53 else 0), rng or _DEFAULT_RNG)


def flagged(top12, add, rng=None):
    """a flagged encoding: the 13 index bits behind top12 are zero, and `add` (1..40; 40: no bit set behind the 25); dense
    rank 13 + add"""
    assert 0 <= top12 < 4096 and 1 <= add <= 40
    bits = min(25 + add, 64)
    return build(_top(bits), (top12 << 52) | ((1 << (39 - add)) if add < 40 else 0), rng or _DEFAULT_RNG)


def plain(top25, rng=None):
    """an unflagged encoding, which is the 25-bit index alone: two calls give two k-mers (almost surely) with one encoding"""
    assert 0 <= top25 < (1 << 25) and top25 & 0x1FFF
    return build(_top(25), top25 << 39, rng or _DEFAULT_RNG)


def first_dense(idx, rank, rng=None):
    """dense() at the first register from idx on, going round, that can hold the rank: (h, v, register)"""
    for i in range(4096):
        try:
            return dense((idx + i) % 4096, rank, rng) + ((idx + i) % 4096,)
        except NoKmer:
            pass
    raise NoKmer(f"rank {rank}")


def first_flagged(top12, add, rng=None):
    for i in range(4096):
        try:
            return flagged((top12 + i) % 4096, add, rng) + ((top12 + i) % 4096,)
        except NoKmer:
            pass
    raise NoKmer(f"add {add}")


def encoding(h):
    """encodeHashIn32Bit (hyperloglogplus.cpp:181-204) for p = 12, p' = 25, restated on Python integers"""
    idx = (h >> 39) << 7
    if (idx << 12) & 0xFFFFFFFF:
        return idx
    rest = (h << 25) & M64
    add = 65 - rest.bit_length() if rest else 40
    return idx | (add << 1) | 1


def dense_rank(h):
    rest = (h << 12) & M64
    return 65 - rest.bit_length() if rest else 53


def ascii_of(v, flip=False, k=K):
    """the k bases of v (the oldest in the high bits), or their reverse complement: both have v as their canonical k-mer"""
    if flip:
        v = revcomp(v, k)
    return bytes(b"ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def reads_of(kmers, per, k=K):
    """reads of `per` k-mers each (the last one of what is left) joined by N, strands alternating: every window across an N is
    ambiguous, so a read books exactly its built k-mers, in order.  k = 31: per = 4 gives 127 bases (97 windows: the fused
    kernel's instances of two items per lane), 5 gives 159 (129 windows: three items), 8 gives 255 (225: the windowed ones)"""
    kmers = list(kmers)
    return [b"N".join(ascii_of(v, (a + j) & 1, k) for j, v in enumerate(kmers[a:a + per])) for a in range(0, len(kmers), per)]
