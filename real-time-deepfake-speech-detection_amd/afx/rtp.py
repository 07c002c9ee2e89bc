"""RTP fixed headers (RFC 3550 section 5.1), as far as a jitter buffer needs them: ``parse`` splits one datagram into
sequence number, timestamp, payload type, SSRC, marker bit and a view of the payload -- past the CSRC list and a header
extension, without the padding the P bit announces.  Nothing is copied.  RTCP, SRTP and payload formats are not this
module's business: ``afx.jitter.JitterScorer.feed_rtp`` maps payload types to the encodings of ``afx.ingest``.
"""
import collections

Packet = collections.namedtuple("Packet", "seq timestamp payload_type ssrc marker payload")

STATIC_PAYLOAD_TYPES = {0: "mulaw", 8: "alaw"}  # RFC 3551: PCMU, PCMA (8 kHz; the RTP clock is the sample rate)
# RFC 3551's static audio payload types a front can score, as (clock rate, encoding): PCMU, DVI4 at its four rates, PCMA and
# mono L16 (network byte order).  10 (stereo L16) is not mapped: channels are not de-interleaved.
STATIC_AUDIO_FORMATS = {0: (8000, "mulaw"), 5: (8000, "dvi4"), 6: (16000, "dvi4"), 8: (8000, "alaw"), 11: (44100, "pcm_s16be"),
                        16: (11025, "dvi4"), 17: (22050, "dvi4")}
CN_PAYLOAD_TYPE = 13  # RFC 3389 comfort noise (8 kHz clock, RFC 3551): payload[0] & 0x7f is the noise level in -dBov; a
# jitter scorer with a ComfortNoise takes it as a silence mark (other clock rates negotiate a dynamic type for it)


def parse(datagram):
    """One RTP datagram (bytes, bytearray or memoryview) -> Packet(seq, timestamp, payload_type, ssrc, marker, payload),
    payload a memoryview into the datagram.  Anything that is not RTP version 2, or whose header, CSRC list, extension or
    padding does not fit the datagram, is a ValueError."""
    if not isinstance(datagram, (bytes, bytearray, memoryview)):
        raise ValueError(f"an RTP datagram is bytes, a bytearray or a memoryview, got {type(datagram).__name__}")
    v = memoryview(datagram)
    if v.ndim != 1 or v.itemsize != 1:
        v = v.cast("B")
    n = len(v)
    if n < 12:
        raise ValueError(f"an RTP datagram has at least 12 bytes, got {n}")
    b0, b1 = v[0], v[1]
    if b0 >> 6 != 2:
        raise ValueError(f"RTP version {b0 >> 6}: only version 2 is read")
    start = 12 + 4 * (b0 & 15)  # the CSRC list
    if start > n:
        raise ValueError("the CSRC list leaves the datagram")
    if b0 & 0x10:  # header extension: 16 bits defined by profile, 16 bits length in 32-bit words, the words
        if start + 4 > n:
            raise ValueError("the header extension leaves the datagram")
        start += 4 + 4 * int.from_bytes(v[start + 2:start + 4], "big")
        if start > n:
            raise ValueError("the header extension leaves the datagram")
    end = n
    if b0 & 0x20:  # padding: the last byte counts the padding bytes, itself included
        pad = v[n - 1] if n > start else 0
        if pad == 0 or pad > n - start:
            raise ValueError("the padding count does not fit the payload")
        end = n - pad
    return Packet(int.from_bytes(v[2:4], "big"), int.from_bytes(v[4:8], "big"), b1 & 0x7F, int.from_bytes(v[8:12], "big"),
                  bool(b1 & 0x80), v[start:end])
