"""The expanded payload codecs of the packet fronts, stated in numpy.

``afx.ingest.ENCODINGS`` are the four encodings every kernel of the fronts indexes by sample.  The codecs here cannot be read
that way -- DVI4 is a recurrence within a packet, the network-order PCM payloads of RFC 3551 need their bytes put together --
so a front expands them first: ``afx_k_payload_expand`` (csrc/afx_packets.hip) writes each packet's samples as fp32 into a
zone of the call's device buffer, and everything downstream reads them there as ``pcm_f32le``.  This module is the statement
the kernel is bit-exact to; every decode is exact in fp32.

  pcm_s16be  big-endian int16 (RTP's L16), v / 32768
  pcm_s24be  big-endian 24-bit two's complement (L24), v / 8388608
  pcm_u8     offset-128 bytes (L8), (b - 128) / 128
  dvi4       RFC 3551 section 4.5.1: a packet is one block: predict (int16, big-endian), index (uint8), one reserved byte,
             then 4-bit codes, the HIGH nibble of each byte first.  The header is the decoder state BEFORE the first code
             (unlike IMA's file blocks, whose header holds the first sample).  A block of B >= 4 bytes holds 2 (B - 4)
             samples.  Per code c:
                 step = STEP[index];  index = clamp(index + IDX[c], 0, 88)
                 d = (step >> 3) + (c & 4 ? step : 0) + (c & 2 ? step >> 1 : 0) + (c & 1 ? step >> 2 : 0)
                 pred = clamp(pred - d if c & 8 else pred + d, -32768, 32767);  the sample is pred / 32768
             A block under 4 bytes, or with a header index above 88, is malformed.

``dvi4_encode`` is the standard IMA encoder, for fixtures, tools and benchmarks; it has no device side.
"""
import numpy as np

CODECS = ("dvi4", "pcm_s16be", "pcm_s24be", "pcm_u8")  # the expand kernel's codec numbers 0..3
UNIT = {"dvi4": 1, "pcm_s16be": 2, "pcm_s24be": 3, "pcm_u8": 1}  # bytes a payload is a whole number of
DVI4_HEADER = 4  # bytes of a DVI4 block before its codes
EXPAND_HDR = 4  # int32 per afx_k_payload_expand row: source byte offset, source bytes, destination byte offset, codec number

STEP = np.array([
    7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143,
    157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411,
    1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442,
    11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767], dtype=np.int32)
IDX = np.array([-1, -1, -1, -1, 2, 4, 6, 8] * 2, dtype=np.int32)


def _codec(codec):
    if codec not in CODECS:
        raise ValueError(f"codec {codec!r}: one of {CODECS}")
    return codec


def _bytes(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    a = np.asarray(data)
    if a.ndim != 1 or a.dtype != np.uint8:
        raise ValueError("a payload is bytes or a 1-D uint8 array")
    return a


def samples(nbytes, codec):
    """The samples a payload of ``nbytes`` bytes of ``codec`` holds; a length no payload of it has is a ValueError."""
    codec, nbytes = _codec(codec), int(nbytes)
    if codec == "dvi4":
        if nbytes < DVI4_HEADER:
            raise ValueError(f"a dvi4 block of {nbytes} bytes is shorter than its {DVI4_HEADER}-byte header")
        return 2 * (nbytes - DVI4_HEADER)
    if nbytes < 0 or nbytes % UNIT[codec]:
        raise ValueError(f"a {codec} packet of {nbytes} bytes splits a {UNIT[codec]}-byte sample")
    return nbytes // UNIT[codec]


def samples_each(nbytes, numbers):
    """``samples`` over int64 arrays of (valid) byte counts and codec numbers."""
    nbytes, numbers = np.asarray(nbytes, dtype=np.int64), np.asarray(numbers, dtype=np.int64)
    unit = np.array([UNIT[c] for c in CODECS], dtype=np.int64)[numbers]
    return np.where(numbers == 0, 2 * (nbytes - DVI4_HEADER), nbytes // unit)


def dvi4_header(block):
    """(predict, index) of a DVI4 block; a malformed one (under 4 bytes, index above 88) is a ValueError."""
    b = _bytes(block)
    if b.size < DVI4_HEADER:
        raise ValueError(f"a dvi4 block of {b.size} bytes is shorter than its {DVI4_HEADER}-byte header")
    if b[2] > 88:
        raise ValueError(f"a dvi4 block with header index {int(b[2])}: at most 88")
    return int(np.int16((int(b[0]) << 8 | int(b[1])) - (65536 if b[0] & 0x80 else 0))), int(b[2])


def dvi4_reference(block):
    """One DVI4 block -> its 2 (B - 4) samples as int16, operation by operation as the module docstring states them."""
    pred, index = dvi4_header(block)
    body = _bytes(block)[DVI4_HEADER:]
    codes = np.stack([body >> 4, body & 15], axis=1).reshape(-1).tolist()  # the high nibble first
    step_of, idx_of = STEP.tolist(), IDX.tolist()
    out = np.empty(len(codes), dtype=np.int16)
    for k, c in enumerate(codes):
        step = step_of[index]
        index = min(max(index + idx_of[c], 0), 88)
        d = (step >> 3) + (step if c & 4 else 0) + (step >> 1 if c & 2 else 0) + (step >> 2 if c & 1 else 0)
        pred = min(max(pred - d if c & 8 else pred + d, -32768), 32767)
        out[k] = pred
    return out


def reference(data, codec):
    """One payload of ``codec`` -> (n,) fp32, the decode the GPU is bit-exact to."""
    codec, b = _codec(codec), _bytes(data)
    n = samples(b.size, codec)
    if codec == "dvi4":
        return dvi4_reference(b).astype(np.float32) / np.float32(32768.0)
    if codec == "pcm_s16be":
        return np.ascontiguousarray(b).view(">i2").astype(np.float32) / np.float32(32768.0)
    if codec == "pcm_u8":
        return (b.astype(np.int32) - 128).astype(np.float32) / np.float32(128.0)
    t = b.reshape(n, 3).astype(np.int32)
    v = (t[:, 0] << 16 | t[:, 1] << 8 | t[:, 2]) - ((t[:, 0] & 0x80) << 17)
    return v.astype(np.float32) / np.float32(8388608.0)


def dvi4_encode(x, state=None):
    """int16 samples -> (one DVI4 block, the state after it): the standard IMA ADPCM encoder started from ``state``
    ((predict, index), default (0, 0)), which the block's header records.  An odd number of samples is a ValueError (a block
    holds whole bytes of codes)."""
    x = np.asarray(x)
    if x.ndim != 1 or x.dtype != np.int16:
        raise ValueError("dvi4_encode: a 1-D int16 array")
    if x.size % 2:
        raise ValueError("dvi4_encode: an even number of samples (two codes per byte)")
    pred, index = (0, 0) if state is None else (int(state[0]), int(state[1]))
    if not -32768 <= pred <= 32767 or not 0 <= index <= 88:
        raise ValueError("dvi4_encode: state is (predict in int16, index in 0..88)")
    head = bytes([(pred >> 8) & 0xFF, pred & 0xFF, index, 0])
    step_of, idx_of = STEP.tolist(), IDX.tolist()
    codes = []
    for v in x.tolist():
        step = step_of[index]
        diff = v - pred
        c = 8 if diff < 0 else 0
        diff = -diff if diff < 0 else diff
        d = step >> 3
        if diff >= step:
            c |= 4
            diff -= step
            d += step
        if diff >= step >> 1:
            c |= 2
            diff -= step >> 1
            d += step >> 1
        if diff >= step >> 2:
            c |= 1
            d += step >> 2
        pred = min(max(pred - d if c & 8 else pred + d, -32768), 32767)
        index = min(max(index + idx_of[c], 0), 88)
        codes.append(c)
    body = bytes(h << 4 | l for h, l in zip(codes[0::2], codes[1::2]))
    return head + body, (pred, index)
