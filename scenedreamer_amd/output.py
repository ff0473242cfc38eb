"""Frame output off the critical path (the reference writes each PNG synchronously inside the render loop,
imaginaire/generators/scenedreamer.py:512-518, :629-631 -- that alone would cap the frame rate).

`FrameWriter.submit(img)` converts the tanh-range image to uint8 on the GPU with the reference's arithmetic
(`((img*0.5+0.5)*255).astype(uint8)`, i.e. truncation), copies it to a pinned host buffer on a side stream and hands
it to worker threads that encode and write the files; the render stream never waits for PCIe, zlib or JPEG.
PNG files are encoded by a small pool (zlib releases the GIL; one thread tops out near 40 frames/s at 960x540); the
video (`video_path`, the reference's `output_dir + '.mp4'` at 10 fps, scenedreamer.py:560, :631) is appended in frame
order by its own thread: through imageio's writer (H.264 via ffmpeg, what the reference produces) where imageio is
importable, else through scenedreamer_amd/mp4.py (Motion-JPEG in an MP4 container, no external dependency).
With `video_backend="mjpeg-gpu"` (opt-in, never chosen by "auto") the JPEG sample is encoded on the GPU from the same uint8 tensor
the PNG is written from (scenedreamer_amd/jpeg.py, csrc/jpeg.hip): only the encoded bytes cross PCIe for the video, the video thread
appends bytes instead of running Pillow's encoder, and with `output_dir=None` the raw frame is not copied to the host at all.
With `png_backend="gpu"` (opt-in; "pillow" is the default and its files are unchanged) the PNG's zlib stream is made on the GPU as well
(scenedreamer_amd/png.py, csrc/png.hip): the side stream encodes, a PNG worker copies exactly the encoded bytes, adds the chunk
framing with its CRC-32 and writes the file; together with "mjpeg-gpu" the raw frame never leaves the device.
`write_scene_maps` writes the two per-trajectory maps of scenedreamer.py:562-563."""
import os
import queue
import threading

import numpy as np
import torch

try:
    from PIL import Image
except ImportError:  # PNG encoding needs Pillow; raw .npy frames are written otherwise
    Image = None


# Colours of the 11 biome / semantic classes in semantic_map.png (data table of scenedreamer.py:532-544, RGB 0..255)
BIOME_COLORS = ((255, 255, 178), (184, 200, 98), (188, 161, 53), (190, 255, 242), (106, 144, 38), (33, 77, 41), (86, 179, 106),
                (34, 61, 53), (35, 114, 94), (0, 0, 255), (0, 255, 0))


def write_scene_maps(output_dir, scene, division="reciprocal"):
    """semantic_map.png (argmax class of current_semantic_map [1,11,S,S] through BIOME_COLORS, RGB) and height_map.png
    (current_height_map [1,1,S,S] as write_img maps it: ((h * 0.5 + 0.5) * 255) truncated to uint8, one channel) --
    scenedreamer.py:545, :562-563.  Returns the two arrays.
    division: the reference pushes the colours through a float round trip (`colours / 255 * 2 - 1` at :544, then write_img's
    `(x * 0.5 + 0.5) * 255` truncated).  `/ 255` on its CUDA tensor is a multiplication by the float32 reciprocal in PyTorch
    ("reciprocal", default: what the reference writes when it runs on a GPU), on a CPU tensor an IEEE division ("ieee"); three
    of the 33 colour values come out one level apart."""
    os.makedirs(output_dir, exist_ok=True)
    sem = torch.argmax(torch.as_tensor(scene.current_semantic_map), dim=1)[0].cpu()
    c = np.asarray(BIOME_COLORS, np.float32)
    c = c * (np.float32(1.0) / np.float32(255.0)) if division == "reciprocal" else c / np.float32(255.0)
    table = torch.from_numpy(c * np.float32(2) - np.float32(1))
    sem_rgb = ((table[sem] * 0.5 + 0.5) * 255).numpy().astype(np.uint8)
    h = torch.as_tensor(scene.current_height_map)[0, 0].cpu().to(torch.float32)
    height = ((h * 0.5 + 0.5) * 255).numpy().astype(np.uint8)
    if Image is not None:
        Image.fromarray(sem_rgb, "RGB").save(os.path.join(output_dir, "semantic_map.png"), compress_level=4)
        Image.fromarray(height, "L").save(os.path.join(output_dir, "height_map.png"), compress_level=4)
    else:
        np.save(os.path.join(output_dir, "semantic_map.npy"), sem_rgb)
        np.save(os.path.join(output_dir, "height_map.npy"), height)
    return sem_rgb, height


class _ImageioVideo:
    """imageio.get_writer(path, fps) with the append / close interface of mp4.Mp4MjpegWriter (scenedreamer.py:560, :631-632)."""

    def __init__(self, path, fps):
        import imageio
        self.w = imageio.get_writer(path, fps=fps)

    def append(self, rgb):
        self.w.append_data(rgb)

    def close(self):
        self.w.close()


def open_video(path, fps=10, backend="auto"):
    """backend: "imageio" (H.264 through ffmpeg, the reference's writer), "mjpeg" (scenedreamer_amd/mp4.py), "mjpeg-gpu" (the same
    container; the caller passes samples already encoded by scenedreamer_amd/jpeg.py to `append_encoded`), or "auto" = imageio if
    it is importable, else mjpeg."""
    if backend in ("auto", "imageio"):
        try:
            return _ImageioVideo(path, fps)
        except Exception:   # noqa: BLE001 -- imageio absent (ImportError), an inert stand-in (AttributeError / NotImplementedError),
            # or present without a video plugin: imageio v3 raises ValueError ("Could not find a backend ...") for .mp4 then
            if backend == "imageio":
                raise
    from .mp4 import Mp4MjpegWriter
    return Mp4MjpegWriter(path, fps=fps)


def to_uint8_hwc(img):
    """[1,3,H,W] in [-1,1] -> uint8 [H,W,3] RGB, same rounding as the reference's write_img (scenedreamer.py:513)."""
    x = ((img * 0.5 + 0.5) * 255).clamp_(0, 255).to(torch.uint8)
    return x[0].permute(1, 2, 0).contiguous()


class MapWriter:
    """One-channel maps off the critical path: the reference's depth/%05d.png (scenedreamer.py:720, :844), written synchronously
    there.  `submit(map, index)` takes a uint8 (bits = 8) or uint16 (bits = 16) [H,W] tensor -- maps.quantise's result -- copies a
    CUDA tensor to a pinned host buffer on a side stream and hands it to `threads` workers that save '%05d.png' as Pillow mode "L" or
    "I;16" at compress_level 4 ('%05d.npy' without Pillow, like FrameWriter); at most `depth` maps are in flight.  `close()` joins
    the workers and re-raises what one of them raised."""

    def __init__(self, output_dir, bits=8, threads=2, depth=8):
        if bits not in (8, 16):
            raise ValueError(f"bits must be 8 or 16, got {bits!r}")
        self.dir, self.bits = output_dir, bits
        os.makedirs(output_dir, exist_ok=True)
        self.dtype = torch.uint8 if bits == 8 else torch.uint16
        self.q = queue.Queue(maxsize=depth)
        self.stream = None                          # made at the first CUDA map, on its device
        self.err = None
        self.maps_done = 0
        self._lock = threading.Lock()
        self.threads = [threading.Thread(target=self._run, daemon=True) for _ in range(max(1, threads))]
        for t in self.threads:
            t.start()

    def submit(self, m, index):
        """Enqueue map `index`; returns immediately (blocks only when `depth` maps are already in flight)."""
        if self.err:
            raise self.err
        if not (isinstance(m, torch.Tensor) and m.dim() == 2 and m.dtype == self.dtype):
            raise ValueError(f"a {self.bits}-bit map writer takes [H,W] tensors of {self.dtype}")
        if m.is_cuda:
            if self.stream is None:
                self.stream = torch.cuda.Stream(m.device)
            m = m.contiguous()
            host = torch.empty(m.shape, dtype=m.dtype, pin_memory=True)
            ready = torch.cuda.Event()
            self.stream.wait_stream(torch.cuda.current_stream(m.device))
            with torch.cuda.stream(self.stream):
                host.copy_(m, non_blocking=True)
                ready.record()
            m.record_stream(self.stream)
        else:
            host, ready = m.contiguous(), None
        self.q.put((index, host, ready))

    def _run(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            index, host, ready = item
            try:
                if ready is not None:
                    ready.synchronize()
                arr = host.numpy()
                if Image is not None:
                    # (a 2-D uint8 array is mode "L"; 16 bits go in as little-endian bytes, which is what "I;16" holds)
                    img = (Image.fromarray(arr) if self.bits == 8 else
                           Image.frombytes("I;16", (arr.shape[1], arr.shape[0]), arr.astype("<u2").tobytes()))
                    img.save(os.path.join(self.dir, f"{index:05d}.png"), compress_level=4)
                else:
                    np.save(os.path.join(self.dir, f"{index:05d}.npy"), arr)
                with self._lock:
                    self.maps_done += 1
            except Exception as e:  # surfaced on the next submit()/close()
                self.err = e
            finally:
                self.q.task_done()

    def close(self):
        for _ in self.threads:
            self.q.put(None)
        for t in self.threads:
            t.join()
        if self.err:
            raise self.err


class FrameWriter:
    def __init__(self, output_dir, fmt="png", png_compress_level=4, depth=8, video_path=None, fps=10, png_threads=3,
                 video_backend="auto", video_quality=92, video_restart_mcus=None, video_slots=2, png_backend="pillow", png_slots=2,
                 png_filter="adaptive"):
        """video_backend: see open_video.  video_quality / video_restart_mcus / video_slots are read by "mjpeg-gpu" only: JPEG
        quality, MCUs per restart interval (None: one MCU row) and the number of scan buffers, i.e. of frames that may be encoded
        but not yet copied to the host (each is sdn_jpeg_scan_bound bytes: 1248 B per 8 x 8 pixels).
        png_backend: "pillow" (Image.save with png_compress_level) or "gpu" (scenedreamer_amd/png.py: needs fmt="png" and CUDA images,
        ignores png_compress_level).  png_slots / png_filter are read by "gpu" only: the number of stream buffers (each is
        sdn_png_stream_bound bytes: 15 bits per byte of the frame) and the PngEncoder's `filter`."""
        if png_backend not in ("pillow", "gpu"):
            raise ValueError(f'png_backend must be "pillow" or "gpu", got {png_backend!r}')
        if png_backend == "gpu" and fmt != "png":
            raise ValueError(f'png_backend="gpu" writes PNG files: fmt must be "png", got {fmt!r}')
        self.dir = output_dir
        if output_dir:
            os.makedirs(output_dir, exist_ok=True)
        self.gpu_png = png_backend == "gpu" and bool(output_dir)
        self.fmt = fmt if (fmt != "png" or Image is not None or self.gpu_png) else "npy"
        self.level = png_compress_level
        self.q = queue.Queue(maxsize=depth)
        self.stream = torch.cuda.Stream() if torch.cuda.is_available() else None
        self.err = None
        self.frames_done = 0
        self._lock = threading.Lock()
        self.threads = [threading.Thread(target=self._run, daemon=True) for _ in range(max(1, png_threads if output_dir else 1))]
        self.video = None
        self.gpu_video = bool(video_path) and video_backend == "mjpeg-gpu"
        self.video_quality, self.video_restart_mcus = int(video_quality), video_restart_mcus
        self._slots = queue.Queue()                 # free (encoder, pinned byte count) pairs, made at the first submit
        self._n_slots = max(1, int(video_slots))
        self._jpeg = None
        self._png_backend, self._png_filter = png_backend, png_filter
        self._pslots = queue.Queue()                # free (PngEncoder, pinned byte count) pairs, made at the first submit
        self._n_pslots = max(1, int(png_slots))
        self._png = None
        self._tls = threading.local()               # each PNG worker's own copy stream
        if video_path:
            self.video = open_video(video_path, fps, video_backend)
            self.vq = queue.Queue(maxsize=depth)
            self.vt = threading.Thread(target=self._run_video, daemon=True)
            self.vt.start()
        for t in self.threads:
            t.start()

    def submit(self, img, index):
        """Enqueue frame `index`; returns immediately (blocks only when `depth` frames are already in flight)."""
        if self.err:
            raise self.err
        if self._png_backend == "gpu" and not img.is_cuda:
            raise ValueError('png_backend="gpu" encodes on the GPU: the image must be a CUDA tensor')
        if self.gpu_video or self.gpu_png:
            return self._submit_gpu(img, index)
        if img.is_cuda:
            u8 = to_uint8_hwc(img)
            host = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
            ready = torch.cuda.Event()
            self.stream.wait_stream(torch.cuda.current_stream(img.device))
            with torch.cuda.stream(self.stream):
                host.copy_(u8, non_blocking=True)
                ready.record()
            u8.record_stream(self.stream)
        else:
            host, ready = to_uint8_hwc(img), None
        if self.video is not None:
            self.vq.put((index, host, ready))
        self.q.put((index, host, ready))

    def _submit_gpu(self, img, index):
        """The form of submit with a GPU encoder ("mjpeg-gpu", png_backend="gpu" or both): the uint8 frame is made once; the side
        stream encodes it (csrc/jpeg.hip, csrc/png.hip) and copies each 4-byte length to pinned memory, and the raw frame only for
        a consumer that still encodes on the CPU (the Pillow PNG pool, or a CPU video backend).  The encoded bytes are copied by the
        video thread / a PNG worker, which alone wait for their length."""
        if not img.is_cuda:
            raise ValueError('video_backend="mjpeg-gpu" encodes on the GPU: the image must be a CUDA tensor')
        u8 = to_uint8_hwc(img)
        H, W = int(u8.shape[0]), int(u8.shape[1])
        if self.gpu_video and self._jpeg is None:
            from . import jpeg
            first = jpeg.JpegEncoder(H, W, self.video_quality, self.video_restart_mcus, device=u8.device)
            self._jpeg = [first] + [jpeg.JpegEncoder(H, W, self.video_quality, self.video_restart_mcus, device=u8.device,
                                                     workspace=first.workspace) for _ in range(self._n_slots - 1)]
            self.vstream = torch.cuda.Stream(u8.device)
            for enc in self._jpeg:
                self._slots.put((enc, torch.zeros(1, dtype=torch.int32, pin_memory=True)))
        if self.gpu_png and self._png is None:
            from . import png
            first = png.PngEncoder(H, W, self._png_filter, device=u8.device)
            self._png = [first] + [png.PngEncoder(H, W, self._png_filter, device=u8.device, workspace=first.workspace)
                                   for _ in range(self._n_pslots - 1)]
            for enc in self._png:
                self._pslots.put((enc, torch.zeros(1, dtype=torch.int32, pin_memory=True)))
        for encs in (self._jpeg, self._png):
            if encs is not None and (H, W) != (encs[0].H, encs[0].W):
                raise ValueError(f"frame size changed: {(encs[0].W, encs[0].H)} -> {(W, H)}")
        # blocks while every buffer of a kind waits for its consumer's copy
        vslot = self._slots.get() if self.gpu_video else None
        pslot = self._pslots.get() if self.gpu_png else None
        raw_for_png = bool(self.dir) and not self.gpu_png
        raw_for_video = self.video is not None and not self.gpu_video
        host = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True) if (raw_for_png or raw_for_video) else None
        ready, vlen_ready, plen_ready = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
        try:
            self.stream.wait_stream(torch.cuda.current_stream(u8.device))
            with torch.cuda.stream(self.stream):
                if vslot is not None:
                    _, nbytes = vslot[0].encode(u8)
                    vslot[1].copy_(nbytes, non_blocking=True)
                    vlen_ready.record()
                if pslot is not None:
                    _, nbytes = pslot[0].encode(u8)
                    pslot[1].copy_(nbytes, non_blocking=True)
                    plen_ready.record()
                if host is not None:
                    host.copy_(u8, non_blocking=True)
                    ready.record()
            u8.record_stream(self.stream)
        except Exception:
            if vslot is not None:
                self._slots.put(vslot)
            if pslot is not None:
                self._pslots.put(pslot)
            raise
        if self.video is not None:
            self.vq.put((index, vslot, vlen_ready) if self.gpu_video else (index, host, ready))
        if self.gpu_png:
            self.q.put((index, pslot, plen_ready))
        elif self.dir:
            self.q.put((index, host, ready))

    def _fetch_png(self, slot, len_ready):
        """PNG worker: wait for the stream length, copy exactly that many bytes to pinned memory on the worker's own stream, free the
        stream buffer for the next encode and return the complete file (the IDAT CRC-32 is computed here, on the host)."""
        from . import png
        enc, nbytes_host = slot
        try:
            len_ready.synchronize()
            n = int(nbytes_host.item()) & 0xFFFFFFFF
            if n > enc.bound:
                raise RuntimeError(f"encoded stream of {n} bytes exceeds the bound of {enc.bound}")
            host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            with torch.cuda.device(enc.device):
                if getattr(self._tls, "stream", None) is None:
                    self._tls.stream = torch.cuda.Stream(enc.device)
                with torch.cuda.stream(self._tls.stream):
                    host.copy_(enc.zstream[:n], non_blocking=True)  # ordered behind the encode by len_ready, which has completed
                    self._tls.stream.synchronize()
        finally:
            self._pslots.put(slot)
        return png.file(enc.H, enc.W, host.numpy().tobytes())

    def _fetch_encoded(self, slot, len_ready):
        """Video thread: wait for the scan length, copy exactly that many scan bytes to pinned memory on the thread's own stream,
        free the scan buffer for the next encode and return the complete JPEG file."""
        from . import jpeg
        enc, nbytes_host = slot
        try:
            len_ready.synchronize()
            n = int(nbytes_host.item()) & 0xFFFFFFFF
            if n > enc.bound:
                raise RuntimeError(f"encoded scan of {n} bytes exceeds the bound of {enc.bound}")
            host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            with torch.cuda.device(enc.device), torch.cuda.stream(self.vstream):
                host.copy_(enc.scan[:n], non_blocking=True)     # ordered behind the encode by len_ready, which has completed
                self.vstream.synchronize()
        finally:
            self._slots.put(slot)
        return enc.header + host.numpy().tobytes() + jpeg.EOI

    def _run(self):
        while True:
            item = self.q.get()
            if item is None:
                return
            index, host, ready = item
            try:
                if self.gpu_png:
                    data = self._fetch_png(host, ready)
                    with open(os.path.join(self.dir, f"{index:05d}.png"), "wb") as f:
                        f.write(data)
                    with self._lock:
                        self.frames_done += 1
                    continue
                if ready is not None:
                    ready.synchronize()
                arr = host.numpy()
                if self.dir:
                    path = os.path.join(self.dir, f"{index:05d}.{self.fmt}")
                    if self.fmt == "png":
                        Image.fromarray(arr, "RGB").save(path, compress_level=self.level)
                    else:
                        np.save(path, arr)
                with self._lock:
                    self.frames_done += 1
            except Exception as e:  # surfaced on the next submit()/close()
                self.err = e
            finally:
                self.q.task_done()

    def _run_video(self):
        """Frames are appended in ascending index order.  Callers normally submit consecutive indices; non-consecutive ones
        (a sharded rank submitting global frame ids f, f + N, ...) or out-of-order ones are handled by a BOUNDED reorder
        buffer: once more than `depth` frames wait for a missing index, the smallest pending index is written and the
        sequence continues from it -- host frames are never held without bound and encoding is never deferred to close()."""
        pending, nxt = {}, None
        limit = max(1, self.vq.maxsize)
        while True:
            item = self.vq.get()
            if item is None:
                for k in sorted(pending):
                    self._append_video(pending[k])
                return
            index, host, ready = item
            try:
                if self.gpu_video:
                    pending[index] = self._fetch_encoded(host, ready)
                else:
                    if ready is not None:
                        ready.synchronize()
                    pending[index] = host.numpy()
                if nxt is None:
                    nxt = index
                while pending:
                    if nxt not in pending:
                        if len(pending) <= limit and min(pending) > nxt:
                            break                       # still plausible that `nxt` arrives
                        nxt = min(pending)              # gap (strided / late indices): continue from the smallest one held
                    self._append_video(pending.pop(nxt))
                    nxt += 1
            except Exception as e:
                self.err = e

    def _append_video(self, frame):
        if self.gpu_video:
            self.video.append_encoded(frame, self._jpeg[0].W, self._jpeg[0].H)
            if not self.dir:                        # video only: no PNG worker sees the frame, so it is counted here
                with self._lock:
                    self.frames_done += 1
        else:
            self.video.append(frame)

    def close(self):
        for _ in self.threads:
            self.q.put(None)
        for t in self.threads:
            t.join()
        if self.video is not None:
            self.vq.put(None)
            self.vt.join()
            self.video.close()
        if self.err:
            raise self.err
