"""BGZF blocks for the tests (test infrastructure): a block of any DEFLATE
form, and the malformed headers every BGZF consumer must refuse -- the host
reader (test_bam.py), the device inflate (test_inflate_gpu.py), the device
fetch (test_fetch_gpu.py) and the header rule itself (bgzf_header_check.c)."""
import struct
import zlib


def bgzf_block(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    z = c.compress(data) + c.flush()
    bsize = 18 + len(z) + 8
    if bsize > 65536:                    # htslib shrinks such an input; not a valid block
        return None
    hdr = struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, bsize - 1)
    return hdr + z + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def malformed_headers(block: bytes):
    """(name, bytes) of six mutations of a valid block from bgzf_block (XLEN 6:
    the BC subfield at bytes 12-17)."""
    def put(at, val):
        b = bytearray(block)
        b[at:at + len(val)] = val
        return bytes(b)
    return [("magic", put(1, bytes([block[1] ^ 1]))),
            ("no FEXTRA", put(3, bytes([block[3] & ~4]))),
            ("no BC subfield", put(13, b"X")),
            ("SLEN 3", put(14, struct.pack("<H", 3))),
            ("BSIZE 10", put(16, struct.pack("<H", 10))),      # smaller than header + footer
            ("cut to 17 bytes", block[:17])]
