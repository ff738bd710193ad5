"""Headless driver: the reference's call order over the mirrored host API.

``Session`` replaces ``EngineMain.cpp:5-23`` + ``Engine.cpp:56-80``: initialise the renderer, load a
scene through ResourceManager (PrepareMeshes -> ImportTexture(skybox) -> ImportMesh... ->
PushMeshesToGPU -> PushTexturesToGPU -> Begin/Register/EndInstanceRegister) and render frames.
It only forwards to ``libcrt_host.so`` / ``libcrt_hip.so``; there is no Python compute path.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import CrtCounters, CrtError, CrtTraceArgs  # noqa: F401 (CrtError is re-exported: driver.CrtError)


class RayHits:
    """The records of Session.trace_rays(mode="closest"): `records` is one (n, 5) int32 tensor on the device holding n CrtRayHit {t, u, v,
    triIndex, instance}; t, u, v (float32) and tri, instance (int32) are views of its columns. A miss: t = 99999, instance = -1, the rest 0."""

    def __init__(self, records, stream=None):
        import torch
        f = records.view(torch.float32)
        self.records = records
        self._stream = stream       # the torch stream the query was enqueued on (None: the caller orders the records itself)
        self.t, self.u, self.v = f[:, 0], f[:, 1], f[:, 2]
        self.tri, self.instance = records[:, 3], records[:, 4]

    def __len__(self):
        return self.records.shape[0]

    def numpy(self):
        """The records on the host as _lib.RAYHIT_DTYPE (synchronises with the stream that produced them)."""
        if self._stream is not None:
            self._stream.synchronize()      # the copy below runs on torch's CURRENT stream, which need not be the query's
        return self.records.cpu().numpy().view(_lib.RAYHIT_DTYPE).reshape(-1)


class SurfaceHits:
    """The records of Session.shade_rays(surface=True): `records` is one (n, 12) int32 tensor on the device holding n CrtSurfaceHit; normal
    (n, 3), t, u, v, tex_u, tex_v (float32) and instance, tri, albedo, material (int32) are views of its columns. A miss: t = 99999,
    instance = -1, the rest 0."""

    def __init__(self, records, stream=None):
        import torch
        f = records.view(torch.float32)
        self.records = records
        self._stream = stream       # the torch stream the query was enqueued on (None: the caller orders the records itself)
        self.normal, self.t = f[:, 0:3], f[:, 3]
        self.instance, self.tri = records[:, 4], records[:, 5]
        self.u, self.v = f[:, 6], f[:, 7]
        self.albedo, self.material = records[:, 8], records[:, 9]
        self.tex_u, self.tex_v = f[:, 10], f[:, 11]

    def __len__(self):
        return self.records.shape[0]

    def numpy(self):
        """The records on the host as _lib.SURFACE_HIT_DTYPE (synchronises with the stream that produced them)."""
        if self._stream is not None:
            self._stream.synchronize()      # the copy below runs on torch's CURRENT stream, which need not be the query's
        return self.records.cpu().numpy().view(_lib.SURFACE_HIT_DTYPE).reshape(-1)


class TemporalHistory:
    """The history of Session.accumulate: two sets of planes (color, moments {m1, m2, N, variance}, geometry {n, t}: (height, width, 4) float32;
    with match_instance=True also instance: (height, width) int32) as torch tensors on the session's device, of which each accumulate reads
    one and writes the other, and the CrttCamera of the set last written. color, moments, geometry, instance: the set last written; frames:
    how many frames went in since the last reset; instances: the CrtMeshInstance records the last frame went in with (accumulate's
    instances=), or None. A history belongs to the session's size at its making: after a resize make a new one."""

    def __init__(self, session, match_instance=False):
        import torch
        if session.host_only or session.multi_device:
            raise ValueError("TemporalHistory: the buffers belong to one GPU; not available in a host-only session or one of several devices")
        self.width, self.height, self.device, self.match_instance = session.width, session.height, session.device, bool(match_instance)
        dev = torch.device("cuda", self.device)
        lib = _lib.temporal()
        planes = [("color", _lib.CRTT_PLANE_COLOR, (4,), torch.float32), ("moments", _lib.CRTT_PLANE_MOMENTS, (4,), torch.float32),
                  ("geometry", _lib.CRTT_PLANE_GEOMETRY, (4,), torch.float32)] + ([("instance", _lib.CRTT_PLANE_INSTANCE, (), torch.int32)] if match_instance else [])
        self.sets = []
        for _ in range(2):
            one = {name: torch.zeros((self.height, self.width) + tail, dtype=dtype, device=dev) for name, _, tail, dtype in planes}
            for name, plane, _, _ in planes:
                assert one[name].numel() * one[name].element_size() == lib.crtt_history_bytes(self.width, self.height, plane), name
            self.sets.append(one)
        self.current, self.camera, self.frames, self.instances = 0, None, 0, None

    def _struct(self, which, camera):
        s = self.sets[which]
        return _lib.CrttHistory(s["color"].data_ptr(), s["moments"].data_ptr(), s["geometry"].data_ptr(),
                                s["instance"].data_ptr() if "instance" in s else None, camera if camera is not None else _lib.CrttCamera())

    color = property(lambda self: self.sets[self.current]["color"])
    moments = property(lambda self: self.sets[self.current]["moments"])
    geometry = property(lambda self: self.sets[self.current]["geometry"])
    instance = property(lambda self: self.sets[self.current].get("instance"))


class Session:
    def __init__(self, width, height, device=0, host_only=False, devices=None):
        """device: one HIP ordinal; devices: a list of ordinals -> several GPUs in this process (Renderer::InitializeDevices;
        the same GPU may be listed more than once to rehearse the multi-device path on a one-GPU box)."""
        self.h = _lib.host()
        self.hip = _lib.hip()
        self.width, self.height = int(width), int(height)
        self.host_only = bool(host_only)
        self.device = int(devices[0]) if devices is not None else int(device)
        self.scene = None
        self.multi_device = devices is not None and len(devices) > 1
        self._last_frame = None     # what the most recent frame came from: "render", "render+gbuffer" or "render_raw" (denoise() asks)
        self._row_bands = False
        self._frame_readers = []    # torch events behind the filters still reading the frame's own buffers (_frame_read_queued)
        if host_only:
            ok = self.h.crth_initialize_host_only(self.width, self.height)
        elif devices is not None:
            ids = (C.c_int * len(devices))(*[int(d) for d in devices])
            ok = self.h.crth_initialize_devices(ids, len(devices), self.width, self.height)
        else:
            ok = self.h.crth_initialize(int(device), self.width, self.height)
        if not ok:
            rc = self.h.crth_last_error()
            raise CrtError(f"Renderer::Initialize failed ({rc}): {self.hip.crt_error_string(rc).decode()}")
        self.open = True

    # ---- lifecycle ----
    def close(self):
        if self.open:
            self._wait_frame_readers()
            self.h.crth_terminate()
            self.open = False

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, what):
        rc = self.h.crth_last_error()
        if rc:
            raise CrtError(f"{what}: error {rc}: {self.hip.crt_error_string(rc).decode()}")

    # ---- the frame's own buffers against the filters that read them ----
    # denoise(), accumulate(), filter_variance(), upsample(), frame_points(), present() and view() hand crt_output_device_ptr() / crt_gbuffer_device_ptr() to a stateless library that
    # enqueues on torch's stream and returns. The session's streams know nothing of that stream, and a synchronous frame always reuses
    # slot 0: the next frame would overwrite, and a resize or close free, what the filter has yet to read. So each such call leaves an
    # event behind it, and whatever writes or frees those buffers waits for the events on the host first, as crt_sync() does for a ray
    # query in flight. (Waiting on the device would take the slot's stream, which the C-ABI keeps to itself.)
    def _frame_read_queued(self):
        """A filter reading the frame's colour buffer or planes was just enqueued on torch's current stream: remember where it ends."""
        import torch
        self._frame_readers = [ev for ev in self._frame_readers if not ev.query()]
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(torch.device("cuda", self.device)))
        self._frame_readers.append(ev)

    def _wait_frame_readers(self):
        """Before the frame's buffers are written or freed: wait, on the host, for the filters still reading them."""
        for ev in self._frame_readers:
            ev.synchronize()
        self._frame_readers = []

    def frame_readers_pending(self):
        """How many filter calls that read the frame's own buffers may still be running (the next render, resize or close waits for them)."""
        self._frame_readers = [ev for ev in self._frame_readers if not ev.query()]
        return len(self._frame_readers)

    # ---- scene ----
    def load_scene(self, scene, device_bvh_build=False):
        h = self.h
        self._wait_frame_readers()
        h.crth_set_device_bvh_build(1 if device_bvh_build else 0)   # BuildBVH on the GPU (same bytes as the host build)
        h.crth_set_asset_root((scene.asset_root or "").encode())
        h.crth_prepare_meshes()
        tex = h.crth_import_texture(scene.skybox.encode())   # must be texture index 2 (Engine.cpp:60-61)
        self._check("ImportTexture(skybox)")
        assert tex == 2, tex
        handles = []
        for path in scene.meshes:
            handles.append(h.crth_import_mesh(path.encode()))
            self._check(f"ImportMesh({path})")
        h.crth_push_meshes()
        h.crth_push_textures()
        self._check("PushMeshesToGPU/PushTexturesToGPU")
        h.crth_begin_instances()
        for inst in scene.instances:
            p, keep = _lib.fptr(inst.matrix)
            h.crth_register_instance(handles[inst.mesh], int(inst.material), p)
        h.crth_end_instances()
        self._check("RegisterMeshInstance")
        self.set_camera(scene.camera_pos, scene.camera_front)
        self.scene = scene
        return handles

    def set_camera(self, pos, front):
        p, k1 = _lib.fptr(np.asarray(pos, np.float32))
        f, k2 = _lib.fptr(np.asarray(front, np.float32))
        self.h.crth_set_camera(p, f)

    def camera(self):
        iv = np.zeros(16, np.float32); ip = np.zeros(16, np.float32); pos = np.zeros(3, np.float32)
        self.h.crth_get_camera(iv.ctypes.data_as(C.POINTER(C.c_float)), ip.ctypes.data_as(C.POINTER(C.c_float)), pos.ctypes.data_as(C.POINTER(C.c_float)))
        return iv, ip, pos

    def resize(self, width, height):
        self._wait_frame_readers()
        self.h.crth_resize(int(width), int(height))
        self._check("OnWindowResize")
        if width >= 16 and height >= 16:
            self.width, self.height = int(width), int(height)
        self._last_frame = None

    # ---- rendering through the mirrored Renderer ----
    def render(self, sun_angle=None, postprocess=False, shadows=False, pipelined=False, refraction=False, fxaa=False, ssaa=1, gbuffer=False):
        if ssaa not in (1, 2, 4):
            raise ValueError(f"ssaa must be 1, 2 or 4, not {ssaa!r}")
        self._wait_frame_readers()
        self.h.crth_set_postprocess(1 if postprocess else 0)
        self.h.crth_set_shadows(1 if shadows else 0)          # extension, off upstream
        self.h.crth_set_refraction(1 if refraction else 0)    # extension, off upstream
        self.h.crth_set_fxaa(1 if fxaa else 0)                # extension: dead code upstream (kernel_main.cl:349)
        self.h.crth_set_supersampling(int(ssaa))              # extension: k x k supersampling, 1, 2 or 4
        self.h.crth_set_gbuffer(1 if gbuffer else 0)          # extension: also write the first-hit planes (read_gbuffer, pick)
        self.h.crth_set_pipelined(1 if pipelined else 0)      # frames in flight; output()/uploads wait
        frame = self.h.crth_render(float(self.scene.sun_angle if sun_angle is None else sun_angle))
        if frame == 0:
            self._check("Renderer::Render")
            raise CrtError("Renderer::Render failed")
        self._last_frame = "render+gbuffer" if gbuffer else "render"
        return frame

    def output(self):
        ptr = self.h.crth_map_output()
        if not ptr:
            self._check("Renderer::MapOutput")
            raise CrtError("Renderer::MapOutput returned null")
        return _lib.as_array(ptr, self.width * self.height * 4, np.float32).reshape(self.height, self.width, 4)

    def read_gbuffer(self):
        """The first-hit planes of the last frame rendered with gbuffer=True (Renderer::MapGBuffer): {"geometry", "ids", "albedo"} ->
        (height, width) arrays of _lib.GBUFFER_GEOMETRY_DTYPE / GBUFFER_IDS_DTYPE / uint32."""
        planes = {}
        for name, (plane, dtype) in _lib.GBUFFER_PLANE_DTYPES.items():
            ptr = self.h.crth_map_gbuffer(plane)
            if not ptr:
                self._raise_and_clear(f"Renderer::MapGBuffer({name})")
            planes[name] = _lib.as_array(ptr, self.width * self.height, dtype).reshape(self.height, self.width)
        return planes

    def pick(self, x, y):
        """What the primary ray of pixel (x, y) hit in that frame (Renderer::PickPixel): one _lib.GBUFFER_PIXEL_DTYPE record."""
        out = np.zeros(1, _lib.GBUFFER_PIXEL_DTYPE)
        if not self.h.crth_pick_pixel(int(x), int(y), out.ctypes.data):
            self._raise_and_clear(f"Renderer::PickPixel({x}, {y})")
        return out[0]

    def _raise_and_clear(self, what):
        # a failed query (no G-buffer frame yet, a pixel outside the frame) must not poison the session's later _check()s
        rc = self.h.crth_last_error()
        self.h.crth_clear_error()
        raise CrtError(f"{what}: error {rc}: {self.hip.crt_error_string(rc).decode()}")

    # ---- direct C-ABI access (same device state the mirror drives) ----
    def trace_args(self, sun_angle=None):
        iv, ip, pos = self.camera()
        a = CrtTraceArgs()
        a.cameraPos[0], a.cameraPos[1], a.cameraPos[2] = float(pos[0]), float(pos[1]), float(pos[2])
        a.time = 0.0
        a.numMeshes = self.h.crth_num_instances()
        a.sunAngle = float(self.scene.sun_angle if sun_angle is None else sun_angle)
        return a, iv, ip

    def render_raw(self, flags=0, sun_angle=None, view=None):
        """crt_render with the session camera, or with explicit `view` = (invView[16], invProj[16], cameraPos[3]) (hazard H10: the
        boundary takes the matrices, so a test may hand it ones no camera produces)."""
        a, iv, ip = self.trace_args(sun_angle)
        if view is not None:
            iv, ip = np.ascontiguousarray(view[0], np.float32).reshape(16), np.ascontiguousarray(view[1], np.float32).reshape(16)
            a.cameraPos[0], a.cameraPos[1], a.cameraPos[2] = (float(x) for x in view[2])
        self._last_frame = "render_raw"
        self._wait_frame_readers()
        _lib.check(self.hip.crt_render(C.byref(a), iv.ctypes.data_as(C.POINTER(C.c_float)), ip.ctypes.data_as(C.POINTER(C.c_float)), int(flags)), "crt_render")

    def sync(self):
        _lib.check(self.hip.crt_sync(), "crt_sync")

    def last_kernel(self):
        """Name(s) of the Trace launch(es) of the most recently submitted frame (crt_debug_last_kernel)."""
        buf = C.create_string_buffer(128)
        _lib.check(self.hip.crt_debug_last_kernel(buf, len(buf)), "crt_debug_last_kernel")
        return buf.value.decode()

    def launch_lists(self, cost, tiles_x, max_split, split_factor, spread=0.0):
        """crt_debug_launch_lists: the feedback sort on chosen per-tile costs, cost of shape (8, slotsPerXcd). Returns (order (8, listCap)
        uint32, listLen (8,) uint32, costAfter (8, slotsPerXcd) uint32)."""
        cost = np.ascontiguousarray(cost, np.uint32)
        S = cost.shape[1]
        order = np.empty((8, S + 3 * 96), np.uint32); length = np.empty(8, np.uint32); after = np.empty((8, S), np.uint32)
        _lib.check(self.hip.crt_debug_launch_lists(cost.ctypes.data, S, int(tiles_x), int(max_split), float(split_factor), float(spread),
                                                   order.ctypes.data, length.ctypes.data, after.ctypes.data), "crt_debug_launch_lists")
        return order, length, after

    def identity_lists(self, slots_per_xcd):
        """crt_debug_launch_lists with -slots_per_xcd: the first frame's identity order, (order (8, listCap), listLen (8,))."""
        S = int(slots_per_xcd)
        order = np.empty((8, S + 3 * 96), np.uint32); length = np.empty(8, np.uint32)
        _lib.check(self.hip.crt_debug_launch_lists(None, -S, 1, 0, 0.0, 0.0, order.ctypes.data, length.ctypes.data, None), "crt_debug_launch_lists")
        return order, length

    def read_launch_lists(self):
        """crt_debug_read_launch_lists: (order (8, listCap) uint32, listLen (8,) uint32, slotsPerXcd) of the lists the next synchronous
        frame would run on; CrtError (CRT_E_UNSUPPORTED) when the session keeps none."""
        length = np.empty(8, np.uint32); S, cap = C.c_int(0), C.c_int(0)
        _lib.check(self.hip.crt_debug_read_launch_lists(None, 0, length.ctypes.data, C.byref(S), C.byref(cap)), "crt_debug_read_launch_lists")
        order = np.empty((8, cap.value), np.uint32)
        _lib.check(self.hip.crt_debug_read_launch_lists(order.ctypes.data, order.size, length.ctypes.data, C.byref(S), C.byref(cap)), "crt_debug_read_launch_lists")
        return order, length, int(S.value)

    def read_output(self):
        out = np.empty((self.height, self.width, 4), np.float32)
        _lib.check(self.hip.crt_read_output(out.ctypes.data, out.size), "crt_read_output")
        return out

    def read_output_rgba8(self):
        """The frame as the bytes of upstream's RGBA8 render target (crt_read_output_rgba8)."""
        out = np.empty((self.height, self.width, 4), np.uint8)
        _lib.check(self.hip.crt_read_output_rgba8(out.ctypes.data, out.size), "crt_read_output_rgba8")
        return out

    def last_gather(self):
        """(bytes, bytes per pixel) the secondary devices sent to the first device for the last frame (crt_debug_last_gather)."""
        b, bpp = C.c_uint64(0), C.c_int(0)
        _lib.check(self.hip.crt_debug_last_gather(C.byref(b), C.byref(bpp)), "crt_debug_last_gather")
        return int(b.value), int(bpp.value)

    def read_gbuffer_raw(self):
        """The same planes through crt_read_gbuffer."""
        planes = {}
        for name, (plane, dtype) in _lib.GBUFFER_PLANE_DTYPES.items():
            out = np.empty((self.height, self.width), dtype)
            _lib.check(self.hip.crt_read_gbuffer(plane, out.ctypes.data, out.nbytes), f"crt_read_gbuffer({name})")
            planes[name] = out
        return planes

    def read_rays(self):
        out = np.empty((self.height, self.width, 3), np.float32)
        _lib.check(self.hip.crt_read_rays(out.ctypes.data, out.size), "crt_read_rays")
        return out

    def counters(self):
        c = CrtCounters()
        _lib.check(self.hip.crt_get_counters(C.byref(c)), "crt_get_counters")
        return c.as_dict()

    def kernel_ms(self, which=2):
        return float(self.hip.crt_last_kernel_ms(int(which)))

    def query_hits(self, origins, dirs):
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros(len(o), _lib.RAYHIT_DTYPE)
        _lib.check(self.hip.crt_query_hits(o.ctypes.data, d.ctypes.data, len(o), self.h.crth_num_instances(), out.ctypes.data), "crt_query_hits")
        return out

    # ---- ray queries on device tensors (Renderer::TraceRays -> crt_trace_rays) ----
    @staticmethod
    def _ray_array(name, x, width):
        """(rows, stride in floats) of a float32 tensor of `width`-vectors: (width,) or (1, width) = one value for every ray (stride 0)."""
        import torch
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise ValueError(f"{name}: a float32 torch tensor is required, not {getattr(x, 'dtype', type(x))}")
        if width == 1:
            if x.dim() != 1 or (x.shape[0] > 1 and x.stride(0) != 1):
                raise ValueError(f"{name}: a contiguous tensor of shape (n,) is required, not shape {tuple(x.shape)}, strides {x.stride()}")
            return x.shape[0], 1
        if x.dim() == 1 and x.shape[0] == width and x.stride(0) == 1:
            return 1, 0
        if x.dim() != 2 or x.shape[1] != width or x.stride(1) != 1:
            raise ValueError(f"{name}: shape (n, {width}) with a contiguous last dimension (or ({width},)) is required, not shape {tuple(x.shape)}, strides {x.stride()}")
        if x.shape[0] == 1 or x.stride(0) == 0:
            return x.shape[0], 0
        if x.stride(0) < width:
            raise ValueError(f"{name}: a row stride of at least {width} floats (or 0) is required, not {x.stride(0)}")
        return x.shape[0], x.stride(0)

    def _ray_arrays(self, items, **tensors):
        """(n, strides) of the tensor arguments of one query, name=(tensor, width): each as _ray_array takes it (None: left out, stride None),
        all of those that are not one shared value with the same number of `items`, all on the session's device."""
        given = {name: (x, self._ray_array(name, x, width)) for name, (x, width) in tensors.items() if x is not None}
        counts = [c for _, (c, st) in given.values() if st != 0 or c == 0]
        n = counts[0] if counts else 1
        if any(c != n for c in counts):
            names = list(tensors)
            raise ValueError(f"{', '.join(names[:-1])} and {names[-1]} disagree about the number of {items}: {counts}")
        for name, (x, _) in given.items():
            if x.device.type != "cuda" or x.device.index != self.device:
                raise ValueError(f"{name}: the tensor is on {x.device}, the session on cuda:{self.device}")
        return n, tuple(given[name][1][1] if name in given else None for name in tensors)

    def trace_rays(self, origins, dirs, tmax=None, mode="closest", inclusive=False):
        """Closest hit ("closest": a RayHits) or occlusion ("occluded": a torch.bool tensor) of n world-space rays given as float32 torch tensors
        on the session's device: origins / dirs of shape (n, 3) -- packed, rows of a wider tensor such as x[:, :3] of (n, 4), or (3,) / (1, 3)
        for one value shared by every ray -- and optionally tmax of shape (n,), the distance bound in units of the direction's length.
        inclusive=True: the inclusive box test (CRT_RAYS_INCLUSIVE, include/crt_api.h) -- a ray enters the boxes it starts in, so a ray from a
        surface sees the mesh it starts on; False: upstream's rule, bit-identical with the frames' traversal.
        Enqueued on torch.cuda.current_stream() without synchronising; the result tensors are ordered on that stream like any torch op."""
        import torch
        if mode not in ("closest", "occluded"):
            raise ValueError(f"mode must be 'closest' or 'occluded', not {mode!r}")
        n, (so, sd, _) = self._ray_arrays("rays", origins=(origins, 3), dirs=(dirs, 3), tmax=(tmax, 1))
        dev = torch.device("cuda", self.device)
        batch = _lib.CrtRayBatch(origins.data_ptr(), dirs.data_ptr(), tmax.data_ptr() if tmax is not None else None, so, sd, n)
        closest = mode == "closest"
        out = torch.empty((n, 5), dtype=torch.int32, device=dev) if closest else torch.empty(n, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        flags = (_lib.CRT_RAYS_CLOSEST if closest else _lib.CRT_RAYS_OCCLUDED) | (_lib.CRT_RAYS_INCLUSIVE if inclusive else 0)
        if not self.h.crth_trace_rays(C.byref(batch), flags, out.data_ptr(), stream.cuda_stream):
            self._raise_and_clear("Renderer::TraceRays")
        return RayHits(out, stream) if closest else out.view(torch.bool)

    def rays_stats(self):
        """(64-ray chunks, chunks traced without the instance cull, workgroups launched) of the last trace_rays, after waiting for it."""
        out = (C.c_uint64 * 3)()
        _lib.check(self.hip.crt_debug_rays_stats(out), "crt_debug_rays_stats")
        return int(out[0]), int(out[1]), int(out[2])

    # ---- shaded ray queries on device tensors (Renderer::ShadeRays -> crt_shade_rays) ----
    def shade_rays(self, origins, dirs, tmax=None, sun_angle=None, radiance=True, surface=False):
        """What a frame computes for a pixel, for n world-space rays given as trace_rays takes them (include/crt_api.h: crt_shade_rays): the
        radiance of both bounces as an (n, 4) float32 tensor (rgb, 1) and / or the first hit's surface record (a SurfaceHits: normal, t, ids,
        barycentrics, albedo, material, uv). tmax bounds the given ray only; sun_angle=None: the scene's. Returns the tensor, the records,
        or (tensor, records) for radiance=True and surface=True. Enqueued on torch.cuda.current_stream() without synchronising."""
        import torch
        if not radiance and not surface:
            raise ValueError("radiance and surface are both False: nothing to compute")
        n, (so, sd, _) = self._ray_arrays("rays", origins=(origins, 3), dirs=(dirs, 3), tmax=(tmax, 1))
        dev = torch.device("cuda", self.device)
        batch = _lib.CrtRayBatch(origins.data_ptr(), dirs.data_ptr(), tmax.data_ptr() if tmax is not None else None, so, sd, n)
        params = _lib.CrtShadeParams(float(self.scene.sun_angle if sun_angle is None else sun_angle), 0)
        rad = torch.empty((n, 4), dtype=torch.float32, device=dev) if radiance else None
        rec = torch.empty((n, 12), dtype=torch.int32, device=dev) if surface else None
        stream = torch.cuda.current_stream(dev)
        if not self.h.crth_shade_rays(C.byref(batch), C.byref(params), rad.data_ptr() if radiance else None, rec.data_ptr() if surface else None,
                                      stream.cuda_stream):
            self._raise_and_clear("Renderer::ShadeRays")
        if radiance and surface:
            return rad, SurfaceHits(rec, stream)
        return rad if radiance else SurfaceHits(rec, stream)

    def shade_stats(self):
        """(64-ray chunks, chunks traced without the instance cull, workgroups launched) of the last shade_rays, after waiting for it."""
        out = (C.c_uint64 * 3)()
        _lib.check(self.hip.crt_debug_shade_stats(out), "crt_debug_shade_stats")
        return int(out[0]), int(out[1]), int(out[2])

    # ---- ambient occlusion (Renderer::TraceAmbientOcclusion / ComputeAmbientOcclusion -> crt_trace_ao / crt_frame_ao) ----
    # radius and bias are lengths in the scene's units and have no default: what counts as "near" is the caller's knowledge of the scene.
    def trace_ao(self, points, normals, samples=8, *, radius, bias, seed=0, inclusive=False):
        """Ambient occlusion (1 = open, 0 = closed; include/crt_api.h) at n points with normals, float32 torch tensors on the session's device
        in the shapes trace_rays takes: (n, 3) packed or as rows of a wider tensor, or (3,) / (1, 3) for one value shared by every point.
        `samples` rays (1, 2, 4, ..., 64) per point reach `radius` far from the point lifted by normal * `bias`. Returns a float32 tensor of
        shape (n,), enqueued on torch.cuda.current_stream() without synchronising. inclusive=True: the sample rays under the inclusive box test
        (CRT_AO_INCLUSIVE), as trace_rays(..., inclusive=True) answers them."""
        import torch
        n, (sp, sn) = self._ray_arrays("points", points=(points, 3), normals=(normals, 3))
        dev = torch.device("cuda", self.device)
        pts = _lib.CrtAoPoints(points.data_ptr(), normals.data_ptr(), sp, sn, n)
        params = _lib.CrtAoParams(int(samples), float(radius), float(bias), int(seed) & 0xFFFFFFFF, _lib.CRT_AO_INCLUSIVE if inclusive else 0, 0.0, 0.0)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        if not self.h.crth_trace_ao(C.byref(pts), C.byref(params), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream):
            self._raise_and_clear("Renderer::TraceAmbientOcclusion")
        return out

    def ambient_occlusion(self, samples=8, *, radius, bias, seed=0, filter=False, depth_tol=0.05, normal_cos=0.9, stream=None, inclusive=False):
        """Ambient occlusion of the pixels of the last frame rendered with gbuffer=True, as a (height, width) float32 array (1 = open; a pixel
        of sky is 1). filter=True: the 5 x 5 mean over neighbours whose distance is within depth_tol (relative) and whose normal's cosine is
        at least normal_cos. `stream`: a hipStream_t as an integer; None: HIP's null stream. inclusive=True: the sample rays under the
        inclusive box test (CRT_AO_INCLUSIVE)."""
        params = _lib.CrtAoParams(int(samples), float(radius), float(bias), int(seed) & 0xFFFFFFFF,
                                  (_lib.CRT_AO_FILTER if filter else 0) | (_lib.CRT_AO_INCLUSIVE if inclusive else 0),
                                  float(depth_tol), float(normal_cos))
        if not self.h.crth_compute_ao(C.byref(params), stream):
            self._raise_and_clear("Renderer::ComputeAmbientOcclusion")
        ptr = self.h.crth_map_ao()
        if not ptr:
            self._raise_and_clear("Renderer::MapAmbientOcclusion")
        return _lib.as_array(ptr, self.width * self.height, np.float32).reshape(self.height, self.width)

    def ao_stats(self):
        """(chunks, chunks traced without the instance cull, workgroups launched) of the last trace_ao / ambient_occlusion, after waiting for it."""
        out = (C.c_uint64 * 3)()
        _lib.check(self.hip.crt_debug_ao_stats(out), "crt_debug_ao_stats")
        return int(out[0]), int(out[1]), int(out[2])

    # ---- what denoise() and accumulate() take: a colour image and the guides beside it ----
    def _image(self, name, x):
        import torch
        H, W = self.height, self.width
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise ValueError(f"{name}: a float32 torch tensor is required, not {getattr(x, 'dtype', type(x))}")
        if tuple(x.shape) != (H, W, 4) or not x.is_contiguous():
            raise ValueError(f"{name}: a contiguous tensor of shape ({H}, {W}, 4) is required, not shape {tuple(x.shape)}, strides {x.stride()}")
        if x.device.type != "cuda" or x.device.index != self.device:
            raise ValueError(f"{name}: the tensor is on {x.device}, the session on cuda:{self.device}")
        return x

    def _guided_frame(self, what, color, surface, guides_only=False):
        """(color, guide layout, geometry, ids, albedo) as device addresses for `what` = "denoise" / "accumulate": color=None is the float
        frame of the last render(gbuffer=True) (waits for the frames in flight first); the guides are that frame's planes, or surface=, a
        SurfaceHits of height * width records. ValueError: see Session.denoise. A caller that was handed a buffer of the frame's own (color is
        None or surface is None) calls _frame_read_queued() behind the launch that reads it. guides_only=True (Session.upsample, whose image
        has another size, and Session.frame_points, which takes no image): `color` is not looked at and the address returned for it is None."""
        H, W = self.height, self.width
        if self.host_only or self.multi_device:
            raise ValueError(f"{what}: the buffers belong to one GPU; not available in a host-only session or one of several devices")
        guides, geometry, ids, albedo = _lib.CRTD_GUIDES_PLANES, None, None, None
        if surface is not None:
            if color is None and not guides_only:
                raise ValueError("surface=: guides for a colour tensor; the frame form (color=None) is guided by the frame's own planes")
            rec = surface.records if isinstance(surface, SurfaceHits) else None
            if rec is None or tuple(rec.shape) != (H * W, 12) or not rec.is_contiguous():
                raise ValueError(f"surface: a SurfaceHits of {H * W} records (height * width, in pixel order) is required")
            if rec.device.type != "cuda" or rec.device.index != self.device:
                raise ValueError(f"surface: the records are on {rec.device}, the session on cuda:{self.device}")
            guides, geometry = _lib.CRTD_GUIDES_SURFACE, rec.data_ptr()
        else:
            if self._row_bands:
                raise ValueError(f"{what}: the session is under row bands; the frame and its planes hold this rank's rows only")
            if self._last_frame != "render+gbuffer":
                raise ValueError(f"{what}: the last frame is no render(gbuffer=True) frame"
                                 + {None: " (none has been rendered since the session began or was resized)", "render": " (it was rendered without gbuffer=True)",
                                    "render_raw": " (it came from render_raw)"}[self._last_frame])
            self.sync()
            geometry, ids, albedo = [self.hip.crt_gbuffer_device_ptr(p) for p in (_lib.CRT_GBUFFER_GEOMETRY, _lib.CRT_GBUFFER_IDS, _lib.CRT_GBUFFER_ALBEDO)]
            if not (geometry and ids and albedo):
                raise CrtError("crt_gbuffer_device_ptr returned null")
        if guides_only:
            return None, guides, geometry, ids, albedo
        if color is None:
            ptr = self.hip.crt_output_device_ptr()
            if not ptr:
                raise CrtError("crt_output_device_ptr returned null")
        else:
            ptr = self._image("color", color).data_ptr()
        return ptr, guides, geometry, ids, albedo

    # ---- denoising on device buffers (libcrt_denoise.so: crtd_denoise; stateless, so there is no Renderer method to mirror) ----
    def denoise(self, color=None, *, iterations=4, depth_tol=0.05, normal_cos=0.9, luma_tol=None, demodulate=True, match_instance=False,
                surface=None, out=None):
        """The edge-avoiding a-trous filter of include/crt_denoise.h: `iterations` passes (1..6) of 5 x 5 taps at steps 1, 2, 4, ..., a tap
        counting when it is a hit whose distance is within depth_tol (relative, times the step) and whose normal's cosine is at least
        normal_cos; luma_tol: also within that luminance of the centre (None: no such stop); demodulate: filter colour / albedo;
        match_instance: taps of the centre's instance only. Returns an (height, width, 4) float32 tensor on the session's device (`out`, when
        given), enqueued on torch.cuda.current_stream() without synchronising.
        color=None: the float frame of the last render(gbuffer=True), guided by its planes (waits for the frames in flight first).
        color given, a contiguous (height, width, 4) float32 tensor on the session's device -- samples accumulated over shade_rays, say --:
        guided by the planes of the last render(gbuffer=True), or by surface=, a SurfaceHits of height * width records from
        shade_rays(surface=True) in pixel order. ValueError: no such frame (none yet, or a later render without gbuffer, a render_raw or a
        resize), a session under row bands or of several devices."""
        import torch
        dev = torch.device("cuda", self.device)
        H, W = self.height, self.width
        frame = _lib.CrtdFrame(W, H, None, _lib.CRTD_GUIDES_PLANES, None, None, None)
        frame.color, frame.guides, frame.geometry, frame.ids, frame.albedo = self._guided_frame("denoise", color, surface)
        result = torch.empty((H, W, 4), dtype=torch.float32, device=dev) if out is None else self._image("out", out)
        params = _lib.CrtdParams(int(iterations), (_lib.CRTD_DEMODULATE if demodulate else 0) | (_lib.CRTD_MATCH_INSTANCE if match_instance else 0)
                                 | (_lib.CRTD_LUMA_STOP if luma_tol is not None else 0), float(depth_tol), float(normal_cos),
                                 float(luma_tol) if luma_tol is not None else 0.0)
        lib = _lib.denoise()
        scratch = torch.empty((H, W, 4), dtype=torch.float32, device=dev) if lib.crtd_scratch_bytes(W, H, params.iterations) else None
        rc = lib.crtd_denoise(C.byref(frame), C.byref(params), result.data_ptr(), scratch.data_ptr() if scratch is not None else None,
                              torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise CrtError(f"crtd_denoise failed with {rc}: {lib.crtd_error_string(rc).decode()}")
        if color is None or surface is None:
            self._frame_read_queued()
        return result      # (scratch goes back to torch's allocator, which hands a block out again in the order of the stream it was made on)

    # ---- temporal accumulation on device buffers (libcrt_temporal.so: crtt_accumulate; stateless: the history is a TemporalHistory) ----
    def accumulate(self, history, color=None, *, surface=None, camera=None, alpha=0.2, moments_alpha=0.2, max_history=32, depth_tol=0.05,
                   normal_cos=0.9, clamp=False, reset=False, instances=None, return_vectors=False):
        """One frame into `history` (a TemporalHistory of this session's size), by the definition of include/crt_temporal.h: the history is
        fetched where each pixel's surface was in the previous frame -- four taps, each counting when it is a hit whose distance is within
        depth_tol (relative) of the reprojected one and whose normal's cosine is at least normal_cos (and, for a history made with
        match_instance=True, of the pixel's instance) -- and blended with the frame: the new frame's share is max(alpha, 1 / N), N counting
        the frames accumulated up to max_history; moments_alpha: the same for the luminance moments; clamp: the history colour is first
        clamped to the frame's 3 x 3 neighbourhood. reset=True (or a history nothing was written to yet) starts over from this frame.
        color, surface: as Session.denoise takes them (None: the float frame of the last render(gbuffer=True), guided by its planes), with the
        same ValueErrors. camera=(invView, invProj, pos): the matrices the frame was shot with; default: self.camera().
        Enqueues on torch.cuda.current_stream() without synchronising, swaps the history's two sets and returns (color, moments): two
        (height, width, 4) float32 tensors, moments = {m1, m2, N, variance} of the luminance. They are the history's own planes: valid until
        the next accumulate but one into it; color is a valid color= for Session.denoise.
        instances=None: the reprojection follows the camera only (libcrt_temporal.so), which is right where no surface moved. instances=: the
        CrtMeshInstance records the frame was rendered with -- an (n,) array of 80-byte records as Session.arenas()["instances"] holds them, or
        (n, 4, 4) float32 inverse transforms -- and the history is fetched where each pixel's instance was in the previous frame, by the
        definition of include/crt_motion.h (libcrt_motion.so): a table of one motion record per instance is made against history.instances, the
        copy kept from the previous accumulate (an instance beyond it is new and has no history), and uploaded on the current stream; the new
        copy is kept in the history. ValueError: records of another shape or dtype; a history whose last frame went in without instances=
        and is not being reset (the previous transforms are unknown). return_vectors=True: returns (color, moments, vectors), vectors a fresh
        (height, width, 4) float32 tensor {fx - x, fy - y, dist, state} per pixel: where the history was fetched relative to the pixel, the
        reprojected distance, and 2 = history kept, 1 = reprojected on the previous screen but no history, 0 (with zeros) = nothing to fetch."""
        import torch
        H, W = self.height, self.width
        if not isinstance(history, TemporalHistory) or (history.width, history.height, history.device) != (W, H, self.device):
            raise ValueError(f"history: a TemporalHistory of {W} x {H} on cuda:{self.device} is required")
        records = None if instances is None else _lib.instance_records(instances)
        if records is not None and not reset and history.camera is not None and history.instances is None:
            raise ValueError("instances=: the history's last frame went in without instances=, so the previous transforms are unknown "
                             "(pass reset=True to start over from this frame)")
        ptr, guides, geometry, ids, _ = self._guided_frame("accumulate", color, surface)
        iv, ip, pos = self.camera() if camera is None else camera
        cam = _lib.crtt_camera(iv, ip, pos, W, H)
        frame = _lib.CrttFrame(W, H, ptr, guides, geometry, ids, cam)
        prev = None if reset or history.camera is None else history._struct(history.current, history.camera)
        nxt = history._struct(1 - history.current, cam)
        params = _lib.CrttParams((_lib.CRTT_MATCH_INSTANCE if history.match_instance else 0) | (_lib.CRTT_CLAMP if clamp else 0), float(alpha),
                                 float(moments_alpha), float(max_history), float(depth_tol), float(normal_cos))
        dev = torch.device("cuda", self.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        vectors = None
        if records is None and not return_vectors:
            lib = _lib.temporal()
            rc = lib.crtt_accumulate(C.byref(frame), None if prev is None else C.byref(prev), C.byref(nxt), C.byref(params), stream)
            if rc != 0:
                raise CrtError(f"crtt_accumulate failed with {rc}: {lib.crtt_error_string(rc).decode()}")
        else:
            lib = _lib.motion()
            table = None        # a reset, or no instances=: every pixel reprojects through the camera alone
            if records is not None and prev is not None and len(records):
                table = torch.from_numpy(_lib.crtm_motions(history.instances, records).view(np.uint8)).to(dev)
            vectors = torch.empty((H, W, 4), dtype=torch.float32, device=dev) if return_vectors else None
            margs = _lib.CrtmMotionArgs(table.data_ptr() if table is not None else None, len(records) if table is not None else 0,
                                        vectors.data_ptr() if return_vectors else None)
            rc = lib.crtm_accumulate(C.byref(frame), None if prev is None else C.byref(prev), C.byref(nxt), C.byref(params), C.byref(margs), stream)
            if rc != 0:
                raise CrtError(f"crtm_accumulate failed with {rc}: {lib.crtm_error_string(rc).decode()}")
            # (table goes back to torch's allocator, which hands a block out again in the order of the stream it was made on)
        if color is None or surface is None:
            self._frame_read_queued()
        history.current, history.camera, history.frames = 1 - history.current, cam, (1 if prev is None else history.frames + 1)
        history.instances = None if records is None else records.copy()
        return (history.color, history.moments, vectors) if return_vectors else (history.color, history.moments)

    def upload_instances(self, records, first=0):
        """crt_upload_instances: replace the instance records from `first` on by `records` -- (n,) CrtMeshInstance records as
        Session.arenas()["instances"] holds them -- for every later frame; it waits for no frame in flight."""
        records = np.asarray(records)
        if records.dtype != _lib.INSTANCE_DTYPE or records.ndim != 1:
            raise ValueError(f"records: an (n,) array of _lib.INSTANCE_DTYPE is required, not dtype {records.dtype}, shape {records.shape}")
        records = np.ascontiguousarray(records)
        _lib.check(self.hip.crt_upload_instances(records.ctypes.data, int(first), len(records)), "crt_upload_instances")

    # ---- variance-guided filtering on device buffers (libcrt_vfilter.so: crtv_filter; stateless, so there is no Renderer method to mirror) ----
    def filter_variance(self, color, moments, *, iterations=4, depth_tol=0.05, normal_cos=0.9, luma_sigma=4.0, luma_floor=1e-4, min_history=4,
                        demodulate=True, match_instance=False, surface=None, out=None, return_variance=False):
        """The variance-guided a-trous filter of include/crt_vfilter.h over what Session.accumulate returns: `color` and `moments`, two contiguous
        (height, width, 4) float32 tensors on the session's device, moments = {m1, m2, N, variance} of the luminance. A pixel's variance is the
        history's where N >= min_history and a 7 x 7 estimate over the moments elsewhere; `iterations` passes (1..5) of 5 x 5 taps at steps 1, 2,
        4, ..., a tap counting when it passes the geometry stops of Session.denoise (depth_tol, normal_cos, match_instance) and its luminance is
        within luma_sigma standard deviations (of the 3 x 3 prefiltered variance) + luma_floor of the centre's, weighted by how far within;
        demodulate: filter colour / albedo. The variance is carried through the passes. Guided as Session.denoise's tensor form is: by the planes
        of the last render(gbuffer=True), or by surface=, a SurfaceHits of height * width records in pixel order; the same ValueErrors.
        Returns an (height, width, 4) float32 tensor (`out`, when given), or (that, the filtered luminance variance as an (height, width) float32
        tensor) with return_variance=True; enqueued on torch.cuda.current_stream() without synchronising."""
        import torch
        dev = torch.device("cuda", self.device)
        H, W = self.height, self.width
        if color is None:
            raise ValueError("color: a tensor is required (Session.accumulate returns it, beside the moments)")
        frame = _lib.CrtvFrame(W, H, None, None, _lib.CRTV_GUIDES_PLANES, None, None, None)
        frame.color, frame.guides, frame.geometry, frame.ids, frame.albedo = self._guided_frame("filter_variance", color, surface)
        frame.moments = self._image("moments", moments).data_ptr()
        result = torch.empty((H, W, 4), dtype=torch.float32, device=dev) if out is None else self._image("out", out)
        variance = torch.empty((H, W), dtype=torch.float32, device=dev) if return_variance else None
        params = _lib.CrtvParams(int(iterations), (_lib.CRTV_DEMODULATE if demodulate else 0) | (_lib.CRTV_MATCH_INSTANCE if match_instance else 0),
                                 float(depth_tol), float(normal_cos), float(luma_sigma), float(luma_floor), float(min_history))
        scratch = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        lib = _lib.vfilter()
        rc = lib.crtv_filter(C.byref(frame), C.byref(params), result.data_ptr(), variance.data_ptr() if return_variance else None, scratch.data_ptr(),
                             torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise CrtError(f"crtv_filter failed with {rc}: {lib.crtv_error_string(rc).decode()}")
        if surface is None:
            self._frame_read_queued()
        return (result, variance) if return_variance else result      # (scratch goes back to torch's allocator, in the order of its stream)

    # ---- guided upsampling on device buffers (libcrt_upsample.so: crtu_upsample; stateless, so there is no Renderer method to mirror) ----
    def upsample(self, low, *, factor=2, offset=(0, 0), surface=None, depth_tol=0.05, normal_cos=0.9, match_instance=False, modulate=False,
                 return_state=False, stream=None):
        """The guided upsample of include/crt_upsample.h: `low`, a pass computed at every `factor`-th pixel (2 or 4) of the frame -- low sample
        (X, Y) sits on pixel (factor * X + offset[0], factor * Y + offset[1]), offset in 0 .. factor-1 -- brought to the frame's resolution by a
        bilinear blend of the up to four samples around each pixel, a sample counting when the pixel it sits on passes the geometry stops of
        Session.denoise against the pixel (depth_tol, relative; normal_cos; match_instance), sky blending among sky; where none counts, the
        sample nearest in depth. `low`: a float32 tensor on the session's device or a numpy array (uploaded on the stream), contiguous, of shape
        (LH, LW) or (LH, LW, 4) with LW = ceil((width - offset[0]) / factor), LH likewise. modulate (four channels): a hit pixel's rgb is
        multiplied by its albedo, for a pass that was traced demodulated. Guided as Session.denoise's tensor form is: by the planes of the last
        render(gbuffer=True) (waits for the frames in flight first), or by surface=, a SurfaceHits of height * width records in pixel order;
        the same ValueErrors. Returns an (height, width) or (height, width, 4) float32 tensor, or (that, the (height, width) int32 state plane:
        0 interpolated, 1 nearest, 2 nothing finite around) with return_state=True; enqueued on `stream`, a torch.cuda.Stream (None:
        torch.cuda.current_stream()), without synchronising."""
        import torch
        dev = torch.device("cuda", self.device)
        H, W = self.height, self.width
        if stream is not None and not isinstance(stream, torch.cuda.Stream):
            raise ValueError(f"stream: a torch.cuda.Stream or None is required, not {type(stream)}")
        factor, (ox, oy) = int(factor), (int(o) for o in offset)
        lib = _lib.upsample()
        lw, lh = C.c_int32(), C.c_int32()
        rc = lib.crtu_low_size(W, H, factor, ox, oy, C.byref(lw), C.byref(lh))
        if rc != 0:
            raise CrtError(f"crtu_low_size failed with {rc}: {lib.crtu_error_string(rc).decode()}")
        frame = _lib.CrtuFrame(W, H, _lib.CRTU_GUIDES_PLANES, None, None, None)
        _, frame.guides, frame.geometry, frame.ids, frame.albedo = self._guided_frame("upsample", None, surface, guides_only=True)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            if isinstance(low, np.ndarray):
                low = torch.from_numpy(np.ascontiguousarray(low)).to(dev)
            shapes = ((lh.value, lw.value), (lh.value, lw.value, 4))
            if not isinstance(low, torch.Tensor) or low.dtype != torch.float32 or tuple(low.shape) not in shapes or not low.is_contiguous():
                raise ValueError(f"low: a contiguous float32 tensor or array of shape {shapes[0]} or {shapes[1]} is required for factor {factor}, "
                                 f"offset {(ox, oy)}, not {getattr(low, 'dtype', type(low))}, shape {tuple(getattr(low, 'shape', ()))}")
            if low.device.type != "cuda" or low.device.index != self.device:
                raise ValueError(f"low: the tensor is on {low.device}, the session on cuda:{self.device}")
            channels = 4 if low.dim() == 3 else 1
            image = _lib.CrtuLow(low.data_ptr(), channels, factor, ox, oy)
            params = _lib.CrtuParams((_lib.CRTU_MATCH_INSTANCE if match_instance else 0) | (_lib.CRTU_MODULATE if modulate else 0), float(depth_tol),
                                     float(normal_cos))
            result = torch.empty((H, W, 4) if channels == 4 else (H, W), dtype=torch.float32, device=dev)
            state = torch.empty((H, W), dtype=torch.int32, device=dev) if return_state else None
            rc = lib.crtu_upsample(C.byref(frame), C.byref(image), C.byref(params), result.data_ptr(), state.data_ptr() if return_state else None,
                                   torch.cuda.current_stream(dev).cuda_stream)
            if rc != 0:
                raise CrtError(f"crtu_upsample failed with {rc}: {lib.crtu_error_string(rc).decode()}")
            if surface is None:
                self._frame_read_queued()
        return (result, state) if return_state else result

    # ---- selective re-tracing on device buffers (libcrt_select.so: crts_compact, crts_points, crts_scatter; stateless like the filters) ----
    def _select_tensor(self, name, x, dtypes, shape=None):
        """`x` checked as an argument of select / frame_points / scatter: a contiguous torch tensor of one of `dtypes` (and of `shape`, where
        given) on the session's device."""
        import torch
        if not isinstance(x, torch.Tensor) or x.dtype not in dtypes:
            raise ValueError(f"{name}: a torch tensor of dtype {' or '.join(str(d) for d in dtypes)} is required, not {getattr(x, 'dtype', type(x))}")
        if not x.is_contiguous() or x.numel() < 1 or (shape is not None and tuple(x.shape) not in shape):
            wanted = "" if shape is None else " of shape " + " or ".join(str(s) for s in shape)
            raise ValueError(f"{name}: a contiguous, non-empty tensor{wanted} is required, not shape {tuple(x.shape)}, strides {x.stride()}")
        if x.device.type != "cuda" or x.device.index != self.device:
            raise ValueError(f"{name}: the tensor is on {x.device}, the session on cuda:{self.device}")
        return x

    def _select_device(self, what):
        import torch
        if self.host_only or self.multi_device:
            raise ValueError(f"{what}: the buffers belong to one GPU; not available in a host-only session or one of several devices")
        return torch.device("cuda", self.device)

    def select(self, words, values=(1, 2), capacity=None):
        """crts_compact (include/crt_select.h): the items of `words` whose value is one of `values` (each 0 .. 31), as an ordered, padded index
        list. `words`: a bool, uint8 or int32 tensor of any shape on the session's device, taken flat -- a mask (True is 1), or the state
        plane of Session.upsample(return_state=True), for which the default `values` name NEAREST and EMPTY. Returns (list, counts), int32
        tensors: list of `capacity` entries (default ceil(n / 8)), the selected flat indices in ascending order and -1 behind them; counts =
        [total, min(total, capacity)]. total > capacity is no error: the first `capacity` are listed. Enqueued on
        torch.cuda.current_stream() without synchronising; nothing here reads counts."""
        import torch
        dev = self._select_device("select")
        words = self._select_tensor("words", words, (torch.bool, torch.uint8, torch.int32))
        mask = 0
        for v in values:
            if not 0 <= int(v) < 32:
                raise ValueError(f"values: each must lie in 0 .. 31, not {v!r}")
            mask |= 1 << int(v)
        n = words.numel()
        capacity = (n + 7) // 8 if capacity is None else int(capacity)
        lib = _lib.select()
        if capacity < 1 or capacity > _lib.CRTS_MAX_ITEMS or n > _lib.CRTS_MAX_ITEMS:
            raise ValueError(f"select: n and capacity must lie in 1 .. 2^28, not n {n}, capacity {capacity}")
        c = _lib.CrtsCompact(words.data_ptr(), words.element_size(), mask, n, capacity)
        lst = torch.empty(capacity, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.crts_scratch_bytes(n) // 4, dtype=torch.int32, device=dev)
        rc = lib.crts_compact(C.byref(c), lst.data_ptr(), counts.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise CrtError(f"crts_compact failed with {rc}: {lib.crts_error_string(rc).decode()}")
        return lst, counts      # (scratch goes back to torch's allocator, which hands a block out again in the order of the stream it was made on)

    def frame_points(self, list=None, *, factor=1, offset=(0, 0), surface=None, dirs=False):
        """crts_points: what Session.trace_ao and the ray queries take, made on the device from the frame's guides. list=None: the pixels a
        low-resolution pass sits on -- item j is low sample (j % LW, j / LW) of Session.upsample's grid for `factor` (1, 2 or 4; 1: every
        pixel) and `offset`. list given, an int32 tensor as Session.select returns it: the listed pixels; an entry that is -1 or names no
        pixel gives all-zero rows, which trace nothing. Returns (positions, normals), or (positions, normals, dirs) with dirs=True: (m, 4)
        float32 tensors -- positions = the hit point and the pixel's distance, normals = the stored normal turned towards the viewer and 0,
        dirs = the pixel's unit ray direction and 0; a pixel that is no hit has a zero point and normal. positions[:, :3] and normals[:, :3]
        are arguments of trace_ao as they are. Guided as Session.upsample is (the last render(gbuffer=True), or surface=), with the same
        ValueErrors; the camera is self.camera(). Enqueued on torch.cuda.current_stream() without synchronising."""
        import torch
        dev = self._select_device("frame_points")
        H, W = self.height, self.width
        lib = _lib.select()
        factor, (ox, oy) = int(factor), (int(o) for o in offset)
        if list is None:
            if factor not in (1, 2, 4) or not (0 <= ox < min(factor, W) and 0 <= oy < min(factor, H)):
                raise ValueError(f"frame_points: factor must be 1, 2 or 4 and offset lie in 0 .. factor-1 inside the frame, not {factor}, {(ox, oy)}")
            count = ((W - ox + factor - 1) // factor) * ((H - oy + factor - 1) // factor)
        else:
            count = self._select_tensor("list", list, (torch.int32,)).numel()
            if list.dim() != 1:
                raise ValueError(f"list: shape (m,) is required, not {tuple(list.shape)}")
        frame = _lib.CrtsFrame(W, H, _lib.CRTS_GUIDES_PLANES, None, _lib.CrttCamera())
        _, frame.guides, frame.geometry, _, _ = self._guided_frame("frame_points", None, surface, guides_only=True)
        iv, ip, pos = self.camera()
        frame.camera = _lib.crtt_camera(iv, ip, pos, W, H)
        items = _lib.CrtsItems(None if list is None else list.data_ptr(), count, factor, ox, oy)
        out = [torch.empty((count, 4), dtype=torch.float32, device=dev) for _ in range(3 if dirs else 2)]
        rc = lib.crts_points(C.byref(frame), C.byref(items), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr() if dirs else None,
                             torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise CrtError(f"crts_points failed with {rc}: {lib.crts_error_string(rc).decode()}")
        if surface is None:
            self._frame_read_queued()
        return tuple(out)

    def scatter(self, list, values, out, state=None):
        """crts_scatter, in place: out.flat[list[j]] = values[j] for every entry of `list` (int32, (m,)) that names an item of `out`; -1 and
        the like are skipped and nothing else is touched. values: float32 (m,) or (m, 4); out: a contiguous float32 tensor of n or n x 4
        elements accordingly, such as an (H, W) or (H, W, 4) image. state: an int32 tensor of n elements whose listed items become 3
        (CRTS_STATE_RETRACED), or None. A list that names an item twice is legal; which value stays is unspecified. Enqueued on
        torch.cuda.current_stream() without synchronising."""
        import torch
        dev = self._select_device("scatter")
        lst = self._select_tensor("list", list, (torch.int32,))
        m = lst.numel()
        if lst.dim() != 1:
            raise ValueError(f"list: shape (m,) is required, not {tuple(lst.shape)}")
        values = self._select_tensor("values", values, (torch.float32,), ((m,), (m, 4)))
        channels = 4 if values.dim() == 2 else 1
        out = self._select_tensor("out", out, (torch.float32,))
        if channels == 4 and (out.dim() < 2 or out.shape[-1] != 4):
            raise ValueError(f"out: four-channel values need a last dimension of 4, not shape {tuple(out.shape)}")
        n = out.numel() // channels
        if state is not None:
            state = self._select_tensor("state", state, (torch.int32,))
            if state.numel() != n:
                raise ValueError(f"state: {n} elements are required, one per item of out, not {state.numel()}")
        if m > _lib.CRTS_MAX_ITEMS or n > _lib.CRTS_MAX_ITEMS:
            raise ValueError(f"scatter: at most 2^28 entries and items, not {m} and {n}")
        lib = _lib.select()
        s = _lib.CrtsScatter(lst.data_ptr(), values.data_ptr(), out.data_ptr(), state.data_ptr() if state is not None else None, m, channels, n,
                             _lib.CRTS_STATE_RETRACED)
        rc = lib.crts_scatter(C.byref(s), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise CrtError(f"crts_scatter failed with {rc}: {lib.crts_error_string(rc).decode()}")

    def retrace_ao(self, ao, state, *, capacity=None, samples=8, radius, bias, seed=0, inclusive=False, surface=None):
        """The consumer of Session.upsample's state plane: the pixels of `ao` (an (height, width) float32 tensor, an upsampled ambient-occlusion
        pass) whose `state` (its (height, width) int32 state plane) is NEAREST or EMPTY are traced at full resolution and patched in place,
        and their state becomes 3. select(state, capacity=) -> frame_points(list) -> trace_ao on all `capacity` items, of which the padding
        traces nothing -> scatter: four calls enqueued on torch.cuda.current_stream() with sizes known on the host, none of which waits.
        capacity: default ceil(height * width / 8). samples, radius, bias, seed, inclusive: as trace_ao takes them (item j of the list is
        point j of that call). surface: as frame_points takes it. Returns counts, the int32 device tensor [total, patched]: the caller reads
        it when it pleases, and total > capacity means that the pixels behind the first `capacity` kept what the upsample gave them."""
        import torch
        self._select_device("retrace_ao")
        H, W = self.height, self.width
        ao = self._select_tensor("ao", ao, (torch.float32,), ((H, W),))
        state = self._select_tensor("state", state, (torch.int32,), ((H, W),))
        lst, counts = self.select(state, (_lib.CRTU_STATE_NEAREST, _lib.CRTU_STATE_EMPTY), capacity)
        positions, normals = self.frame_points(lst, surface=surface)
        values = self.trace_ao(positions[:, :3], normals[:, :3], samples, radius=radius, bias=bias, seed=seed, inclusive=inclusive)
        self.scatter(lst, values, ao, state)
        return counts

    # ---- the end of the chain on device buffers (libcrt_present.so: crtp_present, crtp_view; stateless like the filters) ----
    def _present_outputs(self, dev, out, bytes):
        """(float tensor or None, uint8 tensor or None, what the call returns) for present() and view()."""
        import torch
        H, W = self.height, self.width
        if out is not None:
            self._image("out", out)
        elif not bytes:
            out = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        packed = torch.empty((H, W, 4), dtype=torch.uint8, device=dev) if bytes else None
        return out, packed, (out, packed) if out is not None and bytes else packed if bytes else out

    def present(self, color=None, *, ao=None, ao_strength=1.0, exposure=1.0, postprocess=True, unorm8=True, fxaa=False, heal=False, out=None,
                bytes=True):
        """crtp_present (include/crt_present.h): the stages that follow Trace in a frame -- upstream's RGBA8 render target (unorm8), FXAA (fxaa),
        PostProcess (postprocess), the packed bytes -- applied to `color`, a contiguous (height, width, 4) float32 tensor on the session's
        device such as denoise(), accumulate() or upsample() return; before them rgb * ((1 - ao_strength) + ao_strength * ao) for `ao`, an
        (height, width) float32 tensor, and rgb * exposure; heal: non-finite values become 0 (and a non-finite ao factor 1) first. On the
        plain colour of a frame the result is, bit for bit, what render_raw with the same three flags stores.
        color=None: the float frame of the last render / render_raw (waits for the frames in flight first); ValueError when there is none, in
        a host-only session, one of several devices or one under row bands.
        Returns the (height, width, 4) uint8 tensor of RGBA8 bytes (bytes=True, the default); the (height, width, 4) float32 tensor, alpha 1
        (bytes=False; `out`, when given); or (float tensor, uint8 tensor) when both bytes=True and out= are given. Enqueued on
        torch.cuda.current_stream() without synchronising."""
        import torch
        dev = self._select_device("present")
        H, W = self.height, self.width
        if color is None:
            if self._row_bands:
                raise ValueError("present: the session is under row bands; the frame holds this rank's rows only")
            if self._last_frame is None:
                raise ValueError("present: no frame has been rendered since the session began or was resized")
            self.sync()
            ptr = self.hip.crt_output_device_ptr()
            if not ptr:
                raise CrtError("crt_output_device_ptr returned null")
        else:
            ptr = self._image("color", color).data_ptr()
        if ao is not None:
            ao = self._select_tensor("ao", ao, (torch.float32,), ((H, W),))
        result, packed, returned = self._present_outputs(dev, out, bytes)
        flags = ((_lib.CRTP_UNORM8 if unorm8 else 0) | (_lib.CRTP_POST if postprocess else 0) | (_lib.CRTP_FXAA if fxaa else 0)
                 | (_lib.CRTP_HEAL if heal else 0))
        p = _lib.CrtpPresent(W, H, ptr, ao.data_ptr() if ao is not None else None, float(ao_strength), float(exposure), flags)
        lib = _lib.present()
        nbytes = lib.crtp_scratch_bytes(W, H, flags)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        rc = lib.crtp_present(C.byref(p), result.data_ptr() if result is not None else None, packed.data_ptr() if packed is not None else None,
                              scratch.data_ptr() if scratch is not None else None, torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise CrtError(f"crtp_present failed with {rc}: {lib.crtp_error_string(rc).decode()}")
        if color is None:
            self._frame_read_queued()
        return returned

    def view(self, mode, *, plane=None, surface=None, scale=10.0, lo=0.0, hi=1.0, out=None, bytes=True):
        """crtp_view: a picture of the frame's guides. mode: "normal" (n * 0.5 + 0.5), "depth" (grey scale / (t + scale)), "instance" and
        "triangle" (a hash colour per instance id, per triangle), "albedo" -- guided as Session.upsample is, by the planes of the last
        render(gbuffer=True) or by surface=, a SurfaceHits of height * width records, with the same ValueErrors --, "scalar" (`plane`, an
        (height, width) float32 tensor such as an AO pass, grey from lo to hi, NaN magenta) or "state" (`plane`, the int32 state plane of
        upsample / retrace_ao: interpolated dark grey, nearest orange, empty red, retraced green, anything else magenta). Returns as present()
        does: the uint8 tensor, the float tensor (bytes=False), or both (out= given); both hold the same bytes. Enqueued on
        torch.cuda.current_stream() without synchronising."""
        import torch
        dev = self._select_device("view")
        H, W = self.height, self.width
        if mode not in _lib.CRTP_VIEW_MODES:
            raise ValueError(f"mode: one of {', '.join(_lib.CRTP_VIEW_MODES)} is required, not {mode!r}")
        v = _lib.CrtpView(W, H, _lib.CRTP_GUIDES_PLANES, _lib.CRTP_VIEW_MODES[mode], None, None, None, None, float(scale), float(lo), float(hi))
        planar = mode in ("scalar", "state")
        if planar:
            if surface is not None:
                raise ValueError(f"surface=: the {mode} view reads plane= only")
            v.plane = self._select_tensor("plane", plane, (torch.float32,) if mode == "scalar" else (torch.int32,), ((H, W),)).data_ptr()
        else:
            if plane is not None:
                raise ValueError(f"plane=: the {mode} view reads the frame's guides")
            _, v.guides, v.geometry, v.ids, v.albedo = self._guided_frame("view", None, surface, guides_only=True)
        result, packed, returned = self._present_outputs(dev, out, bytes)
        lib = _lib.present()
        rc = lib.crtp_view(C.byref(v), result.data_ptr() if result is not None else None, packed.data_ptr() if packed is not None else None,
                           torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise CrtError(f"crtp_view failed with {rc}: {lib.crtp_error_string(rc).decode()}")
        if not planar and surface is None:
            self._frame_read_queued()
        return returned

    # ---- metering and auto-exposure on device buffers (libcrt_meter.so: crtx_meter, crtx_expose; stateless like the filters) ----
    def meter(self, color=None, *, ao=None, ao_strength=1.0, key=0.18, low=0.0, high=1.0, min_exposure=2 ** -8, max_exposure=2 ** 8, prev=None,
              rate_up=1.0, rate_down=1.0, region=None, heal=False, histogram=False, groups=0):
        """crtx_meter (include/crt_meter.h): the exposure that brings the average luminance of `color` -- a contiguous (height, width, 4) float32
        tensor on the session's device, composed with `ao` and ao_strength (and healed) as present() composes it -- to `key`, left in device
        memory. The average is the geometric mean (formed in a piecewise-linear log2: up to 6.1 % below it) of the pixels whose luminance is
        finite and not negative, over region=(x0, y0, x1, y1), a half-open rectangle inside the frame (None: all of it); low and high, fractions
        in 0 .. 1, keep only the pixels ranked between them by luminance (by 256 bins, 8 per octave; 0 and 1: every pixel, exactly). The
        exposure is key / average clamped to min_exposure .. max_exposure. prev=: the record of the frame before; the exposure then moves from
        prev's by rate_up (towards a larger one) or rate_down of the way to that target (_lib.meter().crtx_rate(dt, tau) gives a rate from a
        frame time and a time constant), and stays prev's where no pixel is valid. groups: the workgroups of the histogram launch (0: the
        library's choice).
        color=None: the float frame of the last render / render_raw, exactly as present() takes it, with the same ValueErrors.
        Returns the record as an (8,) float32 tensor on the device: [exposure, target, average], then -- through .view(torch.int32) -- meanQ,
        valid, invalid, minQ, maxQ; it is what expose() and prev= take. histogram=True: (record, hist), hist the (256,) int32 counts per bin.
        Enqueued on torch.cuda.current_stream() without synchronising: the host never sees the exposure."""
        import torch
        dev = self._select_device("meter")
        H, W = self.height, self.width
        if color is None:
            if self._row_bands:
                raise ValueError("meter: the session is under row bands; the frame holds this rank's rows only")
            if self._last_frame is None:
                raise ValueError("meter: no frame has been rendered since the session began or was resized")
            self.sync()
            ptr = self.hip.crt_output_device_ptr()
            if not ptr:
                raise CrtError("crt_output_device_ptr returned null")
        else:
            ptr = self._image("color", color).data_ptr()
        if ao is not None:
            ao = self._select_tensor("ao", ao, (torch.float32,), ((H, W),))
        if prev is not None:
            prev = self._select_tensor("prev", prev, (torch.float32,), ((8,),))
        try:
            x0, y0, x1, y1 = (0, 0, W, H) if region is None else (int(v) for v in region)
        except (TypeError, ValueError):
            raise ValueError(f"region: (x0, y0, x1, y1) or None is required, not {region!r}") from None
        lib = _lib.meter()
        groups = int(groups)
        nbytes = lib.crtx_scratch_bytes(W, H, groups)
        if not nbytes:
            raise ValueError(f"groups: 0 .. {_lib.CRTX_MAX_GROUPS} is required, not {groups}")
        record = torch.empty(8, dtype=torch.float32, device=dev)
        hist = torch.empty(_lib.CRTX_HIST_BINS, dtype=torch.int32, device=dev) if histogram else None
        scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        m = _lib.CrtxMeter(W, H, ptr, ao.data_ptr() if ao is not None else None, float(ao_strength),
                           (_lib.CRTX_HEAL if heal else 0) | (_lib.CRTX_ADAPT if prev is not None else 0), x0, y0, x1, y1, float(key), float(low),
                           float(high), float(min_exposure), float(max_exposure), float(rate_up), float(rate_down), groups,
                           prev.data_ptr() if prev is not None else None)
        rc = lib.crtx_meter(C.byref(m), record.data_ptr(), hist.data_ptr() if histogram else None, scratch.data_ptr(),
                            torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise CrtError(f"crtx_meter failed with {rc}: {lib.crtx_error_string(rc).decode()}")
        if color is None:
            self._frame_read_queued()
        return (record, hist) if histogram else record      # (scratch goes back to torch's allocator, in the order of its stream)

    def expose(self, color, record, *, ao=None, ao_strength=1.0, heal=False, out=None):
        """crtx_expose: `color` composed with `ao` (and healed) as present() composes it, times the exposure that `record` -- what meter()
        returned -- holds on the device; alpha stays. present(..., exposure=1.0) of the result then gives what present(color, ao=...,
        exposure=) would with that exposure, which the host never read. Returns the (height, width, 4) float32 tensor (`out`, when given; it
        may be `color`). Enqueued on torch.cuda.current_stream() without synchronising."""
        import torch
        dev = self._select_device("expose")
        H, W = self.height, self.width
        if color is None:
            raise ValueError("color: a tensor is required (meter() takes the frame itself; expose() writes an image of the caller's)")
        ptr = self._image("color", color).data_ptr()
        record = self._select_tensor("record", record, (torch.float32,), ((8,),))
        if ao is not None:
            ao = self._select_tensor("ao", ao, (torch.float32,), ((H, W),))
        result = torch.empty((H, W, 4), dtype=torch.float32, device=dev) if out is None else self._image("out", out)
        e = _lib.CrtxExpose(W, H, ptr, ao.data_ptr() if ao is not None else None, record.data_ptr(), float(ao_strength), _lib.CRTX_HEAL if heal else 0)
        lib = _lib.meter()
        rc = lib.crtx_expose(C.byref(e), result.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        if rc != 0:
            raise CrtError(f"crtx_expose failed with {rc}: {lib.crtx_error_string(rc).decode()}")
        return result

    def set_row_bands(self, band_rows, rank, n_ranks):
        self._wait_frame_readers()
        self.h.crth_set_row_bands(int(band_rows), int(rank), int(n_ranks))
        self._check("SetRowBands")
        self._row_bands = int(n_ranks) > 1

    def owned_rows(self):
        return int(self.hip.crt_owned_rows())

    # ---- host arenas (for the oracle in tests) ----
    def arenas(self):
        h = self.h
        return {
            "tris": _lib.as_array(h.crth_triangles(), h.crth_num_triangles(), _lib.TRI_DTYPE),
            "nodes": _lib.as_array(h.crth_nodes(), h.crth_num_nodes(), _lib.NODE_DTYPE),
            "roots": _lib.as_array(h.crth_roots(), h.crth_num_meshes(), np.uint32),
            "materials": _lib.as_array(h.crth_materials(), 256, _lib.MATERIAL_DTYPE),
            "textures": _lib.as_array(h.crth_textures(), 32, _lib.TEXTURE_DTYPE),
            "texels": _lib.as_array(h.crth_texels(), h.crth_texel_bytes(), np.uint8),
            "instances": _lib.as_array(h.crth_instances(), h.crth_num_instances(), _lib.INSTANCE_DTYPE),
            "num_materials": h.crth_num_materials(),
            "num_textures": h.crth_num_textures(),
        }

    def cpu_raycast(self, origins, dirs, nthreads=1, sse=False):
        """CPU_RayCast over many rays; sse=True: upstream's SSE instruction mix (approximate rcpps), the timing flavour."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros(len(o), _lib.HITRECORD_DTYPE)
        (self.h.crth_cpu_raycast_sse if sse else self.h.crth_cpu_raycast)(o.ctypes.data, d.ctypes.data, len(o), out.ctypes.data, int(nthreads))
        return out
