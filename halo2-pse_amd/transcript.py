"""Host-side restatement of the Blake2b Fiat-Shamir transcript of halo2_proofs::transcript (transcript.rs) for C = bn256::G1Affine,
on Python integers and hashlib:

  Blake2bWrite      :282-286, init / finalize :296-315, write_point / write_scalar :338-351, squeeze_challenge / common_point /
                    common_scalar :368-398
  Blake2bRead       :103-107, init :117-131, read_point / read_scalar :148-175, squeeze_challenge / common_point / common_scalar :206-236
  Challenge255      :486-514: Fr::from_bytes_wide of the 64 hash bytes (the 32-byte repr it keeps is that scalar's)

The hash is Blake2b with a 64-byte digest and the personalisation "Halo2-Transcript" (:123-126); every absorbed message starts with a
prefix byte, BLAKE2B_PREFIX_CHALLENGE / _POINT / _SCALAR (:15-21).  A scalar is an integer in [0, r); a point is (x, y) with integers
in [0, q), or None for the identity, which the transcript refuses as the reference does (:218-223).  Encodings are halo2curves':
a scalar is 32 little-endian bytes of its canonical value (Fr::to_repr); a compressed point is the 32 little-endian bytes of x with
the low bit of y in bit 7 of the last byte, the identity 32 zero bytes (G1Affine::to_bytes, the engine's g1_to_bytes).  Engine
points (Montgomery limbs) pass through g1_to_bytes / g1_from_bytes and point_from_bytes / point_to_bytes here."""
import hashlib

FR_MODULUS = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
FQ_MODULUS = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47

BLAKE2B_PREFIX_CHALLENGE = 0  # :15
BLAKE2B_PREFIX_POINT = 1      # :18
BLAKE2B_PREFIX_SCALAR = 2     # :21
PERSONAL = b"Halo2-Transcript"


class TranscriptError(ValueError):
    """the reference's io::Error: a short proof, an invalid point or scalar encoding, the identity given to common_point"""


def scalar_to_bytes(s):
    """Fr::to_repr"""
    s = int(s)
    if not 0 <= s < FR_MODULUS:
        raise TranscriptError("scalar out of range")
    return s.to_bytes(32, "little")


def scalar_from_bytes(data):
    """Fr::from_repr: None-like failure is a TranscriptError, as read_scalar maps it (:165-170)"""
    if len(data) != 32:
        raise TranscriptError("short read")
    s = int.from_bytes(data, "little")
    if s >= FR_MODULUS:
        raise TranscriptError("invalid field element encoding in proof")
    return s


def on_curve(point):
    """y^2 = x^3 + 3 over Fq, both coordinates canonical; the identity (None) counts"""
    if point is None:
        return True
    x, y = point
    return 0 <= x < FQ_MODULUS and 0 <= y < FQ_MODULUS and (y * y - x * x * x - 3) % FQ_MODULUS == 0


def point_to_bytes(point):
    """G1Affine::to_bytes"""
    if point is None:
        return bytes(32)
    if not on_curve(point):
        raise TranscriptError("point not on the curve")
    x, y = point
    return (x | (y & 1) << 255).to_bytes(32, "little")


def point_from_bytes(data):
    """G1Affine::from_bytes: x below q, x^3 + 3 a square, the root whose low bit is the sign bit; 32 zero bytes are the identity"""
    if len(data) != 32:
        raise TranscriptError("short read")
    v = int.from_bytes(data, "little")
    sign, x = v >> 255, v & ((1 << 255) - 1)
    if x == 0 and sign == 0:
        return None
    if x >= FQ_MODULUS:
        raise TranscriptError("invalid point encoding in proof")
    t = (x * x * x + 3) % FQ_MODULUS
    y = pow(t, (FQ_MODULUS + 1) // 4, FQ_MODULUS)  # q = 3 mod 4
    if y * y % FQ_MODULUS != t:
        raise TranscriptError("invalid point encoding in proof")
    if y & 1 != sign:
        y = FQ_MODULUS - y
    return (x, y)


class _Blake2b:
    """the Transcript impl both views share (:206-236, :368-398)"""

    def __init__(self):
        self.state = hashlib.blake2b(digest_size=64, person=PERSONAL)  # :123-126 / :302-305

    def squeeze_challenge(self):
        """:371-376 and Challenge255::new / get_scalar (:499-513): the scalar itself"""
        self.state.update(bytes([BLAKE2B_PREFIX_CHALLENGE]))
        result = self.state.copy().digest()
        return int.from_bytes(result, "little") % FR_MODULUS  # Fr::from_bytes_wide

    def common_point(self, point):
        """:378-390"""
        if point is None:
            raise TranscriptError("cannot write points at infinity to the transcript")
        if not on_curve(point):
            raise TranscriptError("point not on the curve")
        self.state.update(bytes([BLAKE2B_PREFIX_POINT]))
        self.state.update(int(point[0]).to_bytes(32, "little"))
        self.state.update(int(point[1]).to_bytes(32, "little"))

    def common_scalar(self, scalar):
        """:392-397"""
        data = scalar_to_bytes(scalar)
        self.state.update(bytes([BLAKE2B_PREFIX_SCALAR]))
        self.state.update(data)


class Blake2bWrite(_Blake2b):
    """the prover's view: what is written is absorbed and appended to the proof"""

    def __init__(self):
        super().__init__()
        self.proof = bytearray()

    def write_point(self, point):
        """:341-345"""
        self.common_point(point)
        self.proof += point_to_bytes(point)

    def write_scalar(self, scalar):
        """:346-350"""
        self.common_scalar(scalar)
        self.proof += scalar_to_bytes(scalar)

    def finalize(self):
        """:311-314"""
        return bytes(self.proof)


class Blake2bRead(_Blake2b):
    """the verifier's view over the proof bytes"""

    def __init__(self, proof):
        super().__init__()
        self.proof, self.at = bytes(proof), 0

    def _read(self, n):
        if self.at + n > len(self.proof):
            raise TranscriptError("short read")  # read_exact
        data = self.proof[self.at:self.at + n]
        self.at += n
        return data

    def read_point(self):
        """:151-160"""
        point = point_from_bytes(self._read(32))
        self.common_point(point)
        return point

    def read_scalar(self):
        """:162-174"""
        scalar = scalar_from_bytes(self._read(32))
        self.common_scalar(scalar)
        return scalar

    def remaining(self):
        return len(self.proof) - self.at
