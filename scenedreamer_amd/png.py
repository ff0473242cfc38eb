"""PNG frames encoded on the GPU (csrc/png.hip through sdn_png_encode): the per-frame PNG made from the uint8 [H,W,3] pixels
`output.to_uint8_hwc` returns, in place of the Pillow encode of output.FrameWriter (and through it the reference's write_img,
imaginaire/generators/scenedreamer.py:512-518, :629-631).

8-bit RGB, colour type 2, no interlace.  The device filters the rows (one forced filter type, or per row the type with the smallest
sum of absolute differences), codes them as one dynamic-Huffman deflate block of literals and distance-1 matches with a
literal/length code built from the frame's own histogram, and wraps it as a zlib stream with its Adler-32.  `file` adds the signature,
IHDR, the IDAT framing with its CRC-32 (zlib.crc32 on the host: a device CRC is not implemented) and IEND.  All arithmetic is integer
and specified to the byte: tests/png_ref.py restates it and tests/test_png_gpu.py compares with ==.  There is no CPU substitute:
without the library every call raises."""
import struct
import zlib

import torch

from . import capi, ops

SIGNATURE = b"\x89PNG\r\n\x1a\n"
FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}


def filter_mode(name):
    """"none" | "sub" | "up" | "average" | "paeth" | "adaptive" (or 0 .. 5) -> sdn_png_encode's filter_mode"""
    mode = FILTERS.get(name, name) if isinstance(name, str) else name
    if isinstance(mode, bool) or not isinstance(mode, int) or not 0 <= mode <= 5:
        raise ValueError(f"filter must be one of {sorted(FILTERS, key=FILTERS.get)} or 0 .. 5, got {name!r}")
    return mode


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)))


def file(H, W, zstream_bytes):
    """The complete file: signature, IHDR, one IDAT chunk holding the zlib stream, IEND."""
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"frame size must be 1 .. 65535, got {H} x {W}")
    return (SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", int(W), int(H), 8, 2, 0, 0, 0)) + _chunk(b"IDAT", bytes(zstream_bytes)) +
            _chunk(b"IEND", b""))


def stream_bound(H, W):
    """Bytes the zlib stream of an H x W frame can never exceed (sdn_png_stream_bound)."""
    n = capi.lib().sdn_png_stream_bound(int(H), int(W))
    if n == 0:
        raise ValueError(f"the PNG encoder does not take {H} x {W} frames")
    return n


class PngEncoder:
    """Encoder of H x W frames on `device`; owns the workspace and the stream buffer, so one encode is in flight at a time per encoder
    (the next `encode` on the same stream is ordered behind the reads of the previous result that were enqueued on that stream).
    n_workgroups: launch shape of every kernel (0 = defaults); the bytes do not depend on it.
    workspace: another encoder's workspace of the same frame size, to share it: the two must then encode on one stream."""

    def __init__(self, H, W, filter="adaptive", device="cuda", n_workgroups=0, workspace=None):
        self.H, self.W = int(H), int(W)
        self.filter_mode = filter_mode(filter)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("PngEncoder runs on a GPU: there is no CPU substitute")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_workgroups = int(n_workgroups)
        lib = capi.lib()
        self.bound = stream_bound(self.H, self.W)
        need = lib.sdn_png_workspace_bytes(self.H, self.W)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        elif workspace.dtype != torch.uint8 or workspace.numel() < need or workspace.device != self.device:
            raise ValueError(f"a shared workspace must be a uint8 tensor of >= {need} bytes on {self.device}")
        self.workspace = workspace
        self.zstream = torch.empty(self.bound, dtype=torch.uint8, device=self.device)
        self.nbytes = torch.zeros(1, dtype=torch.int32, device=self.device)       # holds the uint32 byte count

    def encode(self, u8_hwc):
        """uint8 [H,W,3] contiguous on the encoder's device -> (zstream_dev, nbytes_dev): the encoder's own buffers, filled on the
        current stream; nothing is synchronised.  The first nbytes_dev[0] bytes of zstream_dev are the zlib stream."""
        if not (isinstance(u8_hwc, torch.Tensor) and u8_hwc.is_cuda):
            raise RuntimeError("PngEncoder.encode: the frame must be a CUDA tensor")
        if tuple(u8_hwc.shape) != (self.H, self.W, 3):
            raise RuntimeError(f"PngEncoder.encode: expected a [{self.H}, {self.W}, 3] frame, got {tuple(u8_hwc.shape)}")
        ops.png_encode(u8_hwc, self.filter_mode, self.workspace, self.zstream, self.nbytes, self.n_workgroups)
        return self.zstream, self.nbytes

    def encode_to_bytes(self, u8_hwc):
        """The complete file.  Synchronises: a convenience for tests and tools."""
        zstream, nbytes = self.encode(u8_hwc)
        n = int(nbytes.item()) & 0xFFFFFFFF
        return file(self.H, self.W, zstream[:n].cpu().numpy().tobytes())
