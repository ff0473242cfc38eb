"""JPEG frames encoded on the GPU (csrc/jpeg.hip through sdn_jpeg_encode_scan): the video sample of the MJPEG-MP4 writer made
from the uint8 [H,W,3] pixels `output.to_uint8_hwc` returns, in place of the Pillow encode of mp4.Mp4MjpegWriter.append (and through
it the reference's per-frame `fout.append_data(rgb)`, imaginaire/generators/scenedreamer.py:560, :631).

Baseline sequential DCT, 8 bit, three components, 4:4:4 (Pillow's `subsampling=0`), the Annex K quantisation tables scaled by
`quality` as libjpeg scales them and the Annex K Huffman tables.  The scan is cut into restart intervals of `restart_mcus` MCUs
(default: one MCU row) so that it can be encoded in parallel.  The device produces the scan; `header` and EOI are a few hundred bytes
built here.  All arithmetic is integer and specified to the byte: tests/jpeg_ref.py restates it and tests/test_jpeg_gpu.py compares
with ==.  There is no CPU substitute: without the library every call raises."""
import struct

import torch

from . import capi, ops

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
          49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

# ITU-T T.81 Annex K.1 (luminance, chrominance), natural order
QBASE = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)

# ITU-T T.81 Annex K.3: (table class, id) -> (BITS, HUFFVAL); class 0 = DC, 1 = AC; id 0 = luminance, 1 = chrominance
_AC_SYMBOLS = {16 * run + cat for run in range(16) for cat in range(1, 11)} | {0x00, 0xF0}     # what an AC list must hold
HUFFMAN = {
    (0, 0): ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0, 1): ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (1, 0): ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
             (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240,
              36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
              73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131,
              132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
              178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
              217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250)),
    (1, 1): ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
             (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
              21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
              71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
              122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
              168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213,
              214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250)),
}
assert all(sum(b) == len(v) == len(set(v)) for b, v in HUFFMAN.values())
assert all(set(HUFFMAN[(1, t)][1]) == _AC_SYMBOLS for t in (0, 1))

EOI = b"\xff\xd9"


def _check(quality, restart_mcus=1):
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be 1 .. 100, got {quality}")
    if not 1 <= int(restart_mcus) <= 65535:
        raise ValueError(f"restart_mcus must be 1 .. 65535, got {restart_mcus}")


def quant_tables(quality):
    """(luminance, chrominance): 64 integers each in natural order -- the Annex K tables scaled like libjpeg's jpeg_set_quality:
    s = 5000 // quality below 50, else 200 - 2 quality; entry = clamp((base s + 50) // 100, 1, 255)."""
    _check(quality)
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(255, max(1, (b * s + 50) // 100)) for b in base) for base in QBASE)


def default_restart_mcus(W):
    """One MCU row."""
    return -(-int(W) // 8)


def _segment(marker, payload):
    return bytes((0xFF, marker)) + struct.pack(">H", len(payload) + 2) + payload


def header(H, W, quality, restart_mcus):
    """SOI, APP0 (JFIF 1.01, no units, 1:1), DQT 0, DQT 1, SOF0, DHT x 4 (DC 0, AC 0, DC 1, AC 1), DRI, SOS: everything before the scan."""
    _check(quality, restart_mcus)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"frame size must be 1 .. 65535, got {H} x {W}")
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + bytes((1, 1, 0)) + struct.pack(">HH", 1, 1) + bytes((0, 0)))]
    for t, q in enumerate(quant_tables(quality)):
        out.append(_segment(0xDB, bytes((t,)) + bytes(q[z] for z in ZIGZAG)))
    out.append(_segment(0xC0, bytes((8,)) + struct.pack(">HH", H, W) + bytes((3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1))))
    for key in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bits, vals = HUFFMAN[key]
        out.append(_segment(0xC4, bytes((key[0] << 4 | key[1],)) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDD, struct.pack(">H", int(restart_mcus))))
    out.append(_segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))))
    return b"".join(out)


def scan_bound(H, W, restart_mcus):
    """Bytes the scan of an H x W frame can never exceed (sdn_jpeg_scan_bound)."""
    n = capi.lib().sdn_jpeg_scan_bound(int(H), int(W), int(restart_mcus))
    if n == 0:
        raise ValueError(f"the JPEG encoder does not take {H} x {W} frames with restart_mcus = {restart_mcus}")
    return n


class JpegEncoder:
    """Encoder of H x W frames on `device`; owns the workspace and the scan buffer, so one encode is in flight at a time per encoder
    (the next `encode` on the same stream is ordered behind the reads of the previous result that were enqueued on that stream).
    n_workgroups: launch shape of every kernel (0 = defaults); the bytes do not depend on it.
    workspace: another encoder's workspace of the same frame size and interval, to share it: the two must then encode on one stream."""

    def __init__(self, H, W, quality=92, restart_mcus=None, device="cuda", n_workgroups=0, workspace=None):
        self.H, self.W, self.quality = int(H), int(W), int(quality)
        self.restart_mcus = default_restart_mcus(W) if restart_mcus is None else int(restart_mcus)
        _check(self.quality, self.restart_mcus)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("JpegEncoder runs on a GPU: there is no CPU substitute")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_workgroups = int(n_workgroups)
        lib = capi.lib()
        self.bound = scan_bound(self.H, self.W, self.restart_mcus)
        self.header = header(self.H, self.W, self.quality, self.restart_mcus)
        need = lib.sdn_jpeg_workspace_bytes(self.H, self.W, self.restart_mcus)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        elif workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != self.device:
            raise ValueError(f"a shared workspace must be a uint8 tensor of >= {need} bytes on {self.device}")
        self.workspace = workspace
        self.scan = torch.empty(self.bound, dtype=torch.uint8, device=self.device)
        self.nbytes = torch.zeros(1, dtype=torch.int32, device=self.device)       # holds the uint32 byte count

    def encode(self, u8_hwc):
        """uint8 [H,W,3] contiguous on the encoder's device -> (scan_dev, nbytes_dev): the encoder's own buffers, filled on the
        current stream; nothing is synchronised.  The first nbytes_dev[0] bytes of scan_dev are the scan."""
        if not (isinstance(u8_hwc, torch.Tensor) and u8_hwc.is_cuda):
            raise RuntimeError("JpegEncoder.encode: the frame must be a CUDA tensor")
        if tuple(u8_hwc.shape) != (self.H, self.W, 3):
            raise RuntimeError(f"JpegEncoder.encode: expected a [{self.H}, {self.W}, 3] frame, got {tuple(u8_hwc.shape)}")
        ops.jpeg_encode_scan(u8_hwc, self.quality, self.restart_mcus, self.workspace, self.scan, self.nbytes, self.n_workgroups)
        return self.scan, self.nbytes

    def encode_to_bytes(self, u8_hwc):
        """The complete file (header + scan + EOI).  Synchronises: a convenience for tests and tools."""
        scan, nbytes = self.encode(u8_hwc)
        n = int(nbytes.item()) & 0xFFFFFFFF
        return self.header + scan[:n].cpu().numpy().tobytes() + EOI
