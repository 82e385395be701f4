"""The Blake2b transcript of transcript.py against the format as transcript.rs states it, worked out here with hashlib and Python
integers: Blake2b-512 personalised "Halo2-Transcript"; a point is absorbed as the byte 1, then x and y as 32 little-endian bytes each; a
scalar as the byte 2 and its 32 little-endian bytes; a challenge absorbs the byte 0, and is the little-endian integer of the 64 digest
bytes of a copy of the state, reduced mod r.  No GPU."""
import hashlib

import pytest

from proof_util import G1, Q, g1_mul, transcript as tr

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
POINTS = [g1_mul(G1, 5), g1_mul(G1, R - 1), g1_mul(G1, 0x1234567890ABCDEF1234567890ABCDEF)]
SCALARS = [0, 1, R - 1, 0xDEADBEEF << 200]


def le32(v):
    return int(v).to_bytes(32, "little")


def test_the_generator_multiples_are_on_the_curve():
    for x, y in POINTS:
        assert (y * y - x * x * x - 3) % Q == 0
    assert g1_mul(G1, R) is None


def test_challenges_equal_the_format_restated_with_hashlib():
    w = tr.Blake2bWrite()
    ref = hashlib.blake2b(digest_size=64, person=b"Halo2-Transcript")
    got, want = [], []

    def squeeze():
        got.append(w.squeeze_challenge())
        ref.update(b"\x00")
        want.append(int.from_bytes(ref.copy().digest(), "little") % R)

    squeeze()  # a challenge of the empty transcript
    w.common_scalar(SCALARS[3])
    ref.update(b"\x02" + le32(SCALARS[3]))
    w.write_point(POINTS[0])
    ref.update(b"\x01" + le32(POINTS[0][0]) + le32(POINTS[0][1]))
    squeeze()
    squeeze()  # two in a row differ: the prefix byte stays absorbed
    for s in SCALARS[:3]:
        w.write_scalar(s)
        ref.update(b"\x02" + le32(s))
    w.common_point(POINTS[1])
    ref.update(b"\x01" + le32(POINTS[1][0]) + le32(POINTS[1][1]))
    w.write_point(POINTS[2])
    ref.update(b"\x01" + le32(POINTS[2][0]) + le32(POINTS[2][1]))
    squeeze()
    assert got == want
    assert len(set(got)) == 4 and all(0 <= c < R for c in got)
    # the proof holds what was written, not what was common: one compressed point, three scalars, one compressed point
    x0, y0 = POINTS[0]
    x2, y2 = POINTS[2]
    assert w.finalize() == le32(x0 | (y0 & 1) << 255) + b"".join(le32(s) for s in SCALARS[:3]) + le32(x2 | (y2 & 1) << 255)


def test_write_then_read_round_trips():
    w = tr.Blake2bWrite()
    c_w = []
    for p, s in zip(POINTS, SCALARS):
        w.write_point(p)
        c_w.append(w.squeeze_challenge())
        w.write_scalar(s)
    c_w.append(w.squeeze_challenge())
    proof = w.finalize()
    assert len(proof) == 64 * len(POINTS)
    r = tr.Blake2bRead(proof)
    c_r = []
    for p, s in zip(POINTS, SCALARS):
        assert r.read_point() == p
        c_r.append(r.squeeze_challenge())
        assert r.read_scalar() == s
    c_r.append(r.squeeze_challenge())
    assert c_r == c_w and r.remaining() == 0
    with pytest.raises(tr.TranscriptError, match="short read"):
        r.read_scalar()


def test_both_signs_of_y_round_trip():
    x, y = POINTS[0]
    for p in ((x, y), (x, Q - y)):
        assert tr.point_from_bytes(tr.point_to_bytes(p)) == p
    assert tr.point_to_bytes((x, y)) != tr.point_to_bytes((x, Q - y))
    assert tr.point_from_bytes(bytes(32)) is None and tr.point_to_bytes(None) == bytes(32)


def test_read_rejects_what_the_reference_rejects():
    # x = 4: 4^3 + 3 = 67 is checked below not to be a square mod q, so no point has this x
    assert pow(67, (Q - 1) // 2, Q) == Q - 1
    with pytest.raises(tr.TranscriptError, match="invalid point encoding"):
        tr.Blake2bRead(le32(4)).read_point()
    with pytest.raises(tr.TranscriptError, match="invalid point encoding"):
        tr.Blake2bRead(le32(Q)).read_point()  # x = q: not canonical
    for s in (R, R + 5, (1 << 256) - 1):
        with pytest.raises(tr.TranscriptError, match="invalid field element encoding"):
            tr.Blake2bRead(le32(s)).read_scalar()
    assert tr.Blake2bRead(le32(R - 1)).read_scalar() == R - 1
    with pytest.raises(tr.TranscriptError, match="short read"):
        tr.Blake2bRead(bytes(31)).read_point()
    # the identity decodes, and the transcript refuses to absorb it
    with pytest.raises(tr.TranscriptError, match="infinity"):
        tr.Blake2bRead(bytes(32)).read_point()


def test_write_rejects_what_cannot_be_absorbed():
    w = tr.Blake2bWrite()
    x, y = POINTS[0]
    with pytest.raises(tr.TranscriptError):
        w.write_point((x, (y + 1) % Q))  # not on the curve
    with pytest.raises(tr.TranscriptError):
        w.write_point(None)
    for s in (R, -1):
        with pytest.raises(tr.TranscriptError):
            w.write_scalar(s)
    assert w.finalize() == b""
