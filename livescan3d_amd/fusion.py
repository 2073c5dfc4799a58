"""Device-resident fusion on torch-allocated HBM buffers (torch is plumbing only: memory, streams)."""
import numpy as np
import torch

from . import native

SENTINEL = -7   # prefill of both offset tables: no legal offset, so an entry that was never written shows


def _stream_handle(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def _device(device=None):
    return torch.device("cuda", torch.cuda.current_device() if device is None else device)


class DeviceFusion:
    """T ticks x N sensors -> T merged clouds (and meshes), inputs and outputs resident in HBM: the one device batch of the tests and tools.

    depth: torch.int16 / uint16-bit-pattern tensor [T, sum(w*h)] (or any shape with that many u16 per tick),
    rgb:   torch.uint8 tensor [T, sum(w*h)*3]; from_rigs() uploads them, and every launch takes another pair in their place.
    Outputs, owned by the object: vertices torch.uint8 [T, capacity, 16] viewed as VertexC4ubV3f, offsets torch.int32 [T, N+1]
    (offsets[k, i] = first vertex of sensor i, offsets[k, N] = nVertices); triangles torch.int32 [T, 2*capacity, 3] and tri_offsets
    [T, N+1], allocated when first needed.  Both offset tables are prefilled with SENTINEL.  The methods launch on the current stream (or
    `stream`, a torch stream) and return at once; the host views at the end synchronise.  Nothing here checks a result."""

    def __init__(self, n_ticks, widths, heights, device=None, mode=0):
        if not torch.cuda.is_available():
            raise native.NativeUtilsError("DeviceFusion needs a HIP device (no CPU path)")
        self.device = _device(device)
        self.plan = native.FusionPlan(self.device.index, n_ticks, widths, heights)
        self.plan.set_mode(mode)
        self.n_ticks, self.n_maps = n_ticks, self.plan.n_maps
        self.capacity = self.plan.capacity
        # (not cleared here: the benchmark and the drivers construct their plans this way; from_rigs() clears them)
        self.vertices = torch.empty((n_ticks, self.capacity, 16), dtype=torch.uint8, device=self.device)
        self.offsets = torch.full((n_ticks, self.n_maps + 1), SENTINEL, dtype=torch.int32, device=self.device)
        self.depth = self.rgb = self.intr = self._triangles = self._tri_offsets = self._normals = self._smoothed = None

    @classmethod
    def from_rigs(cls, rigs, n_ticks=None, device=None, mode=0):
        """A plan of n_ticks (default len(rigs)) ticks of rigs[0]'s sizes with rigs[k % len(rigs)] uploaded as tick k and the vertices
        cleared.  One calibration for the plan: intr, wt and bounds are rigs[0]'s, whatever the other rigs carry."""
        self = cls(len(rigs) if n_ticks is None else n_ticks, rigs[0].widths, rigs[0].heights, device, mode)
        self.set_params(rigs[0].intr, rigs[0].wt, rigs[0].bounds)
        self.depth, self.rgb = upload_rigs(rigs, self.n_ticks, self.device.index)
        self.vertices.zero_()
        return self

    @property
    def tiles_per_tick(self):
        return self.plan.tiles_per_tick

    def _mesh(self):
        if self._triangles is None:
            self._triangles = torch.zeros((self.n_ticks, 2 * self.capacity, 3), dtype=torch.int32, device=self.device)
            self._tri_offsets = torch.full((self.n_ticks, self.n_maps + 1), SENTINEL, dtype=torch.int32, device=self.device)
        return self._triangles, self._tri_offsets

    @property
    def triangles(self):
        return self._mesh()[0]

    @property
    def tri_offsets(self):
        return self._mesh()[1]

    def set_params(self, intr, wt, bounds):
        self.intr = intr
        self.plan.set_params(intr, wt, bounds, _stream_handle())

    def _in(self, depth, rgb=None):
        """The data pointers of the inputs of a launch: the tensors handed in, else the uploaded ticks."""
        return (self.depth if depth is None else depth).data_ptr(), (self.rgb if rgb is None else rgb).data_ptr()

    def run(self, depth=None, rgb=None, stream=None):
        depth, rgb = self.depth if depth is None else depth, self.rgb if rgb is None else rgb
        assert depth.is_cuda and rgb.is_cuda and depth.is_contiguous() and rgb.is_contiguous()
        assert depth.element_size() == 2 and depth.numel() == self.n_ticks * self.plan.pixels_per_tick, depth.shape
        assert rgb.dtype == torch.uint8 and rgb.numel() == self.n_ticks * self.plan.pixels_per_tick * 3, rgb.shape
        self.plan.run(depth.data_ptr(), rgb.data_ptr(), self.vertices.data_ptr(), self.offsets.data_ptr(), _stream_handle(stream))
        return self.vertices, self.offsets

    def run_mesh(self, depth=None, rgb=None, stream=None):
        self.plan.run_mesh(*self._in(depth, rgb), self.vertices.data_ptr(), self.offsets.data_ptr(), self.triangles.data_ptr(),
                           self.tri_offsets.data_ptr(), _stream_handle(stream))

    def radial_correct(self, depth=None, rgb=None, stream=None, intr=None):
        """In place, on the uploaded ticks unless another pair is handed in; intr: the plan's unless given."""
        self.plan.radial_correct(self.intr if intr is None else intr, *self._in(depth, rgb), _stream_handle(stream))

    def radial_correct_to(self, depth_out, rgb_out, depth=None, rgb=None, stream=None, intr=None):
        self.plan.radial_correct_to(self.intr if intr is None else intr, *self._in(depth, rgb), depth_out.data_ptr(), rgb_out.data_ptr(),
                                    _stream_handle(stream))

    def color_transfer(self, depth=None, stream=None):
        self.plan.color_transfer(self._in(depth)[0], self.vertices.data_ptr(), self.offsets.data_ptr(), _stream_handle(stream))

    def color_blend(self, depth_tol, min_confidence, depth=None, stream=None):
        """Colour blending across views in place on the batch's vertices (behind color_transfer() when both run)."""
        self.plan.color_blend(depth_tol, min_confidence, self._in(depth)[0], self.vertices.data_ptr(), self.offsets.data_ptr(),
                              _stream_handle(stream))

    def color_blend_diagnostics(self, tick=0, stream=None):
        return self.plan.color_blend_diagnostics(tick, _stream_handle(stream))

    def overlay_merge(self, depth=None, stream=None):
        self.plan.overlay_merge(self._in(depth)[0], self.vertices.data_ptr(), self.offsets.data_ptr(), self.triangles.data_ptr(),
                                self.tri_offsets.data_ptr(), _stream_handle(stream))

    def outlier_filter(self, k, max_dist, depth_out, depth=None, stream=None):
        self.plan.outlier_filter(k, max_dist, self._in(depth)[0], self.vertices.data_ptr(), self.offsets.data_ptr(), depth_out.data_ptr(),
                                 _stream_handle(stream))

    def flying_pixels(self, neighbourhood, threshold, depth_out, depth=None, stream=None):
        self.plan.flying_pixels(neighbourhood, threshold, self._in(depth)[0], depth_out.data_ptr(), _stream_handle(stream))

    def depth_smooth(self, depth_out, depth=None, stream=None):
        """Depth smoothing with the tables of plan.set_depth_smooth(), out of place into depth_out."""
        self.plan.depth_smooth(self._in(depth)[0], depth_out.data_ptr(), _stream_handle(stream))

    def set_temporal(self, alpha_q, delta=0, persist=0):
        self.plan.set_temporal(alpha_q, delta, persist)

    def temporal(self, depth_out, depth=None, stream=None):
        """The temporal depth filter with the setting of set_temporal() on the batch's ticks in order, into depth_out (which may be the
        input itself: in place); the plan's history advances by the batch's ticks."""
        self.plan.temporal(self._in(depth)[0], depth_out.data_ptr(), _stream_handle(stream))

    def temporal_reset(self, stream=None):
        self.plan.temporal_reset(_stream_handle(stream))

    def temporal_state(self, stream=None):
        return self.plan.temporal_state(_stream_handle(stream))

    def set_temporal_state(self, state, stream=None):
        self.plan.set_temporal_state(state, _stream_handle(stream))

    def temporal_diagnostics(self, tick=0, stream=None):
        return self.plan.temporal_diagnostics(tick, _stream_handle(stream))

    def set_background(self, margin, rel_q=0, min_pixels=0):
        self.plan.set_background(margin, rel_q, min_pixels)

    def background_learn(self, depth=None, stream=None):
        """Folds the batch's ticks into the plan's background model."""
        self.plan.background_learn(self._in(depth)[0], _stream_handle(stream))

    def background(self, depth_out, depth=None, stream=None):
        """Background subtraction with the setting of set_background() against the plan's model, into depth_out (which may be the input
        itself: in place)."""
        self.plan.background(self._in(depth)[0], depth_out.data_ptr(), _stream_handle(stream))

    def background_reset(self, stream=None):
        self.plan.background_reset(_stream_handle(stream))

    def background_model(self, stream=None):
        return self.plan.background_model(_stream_handle(stream))

    def set_background_model(self, model, stream=None):
        self.plan.set_background_model(model, _stream_handle(stream))

    def background_diagnostics(self, tick=0, stream=None):
        return self.plan.background_diagnostics(tick, _stream_handle(stream))

    def render_views(self, intr, wt, width, height, points=False, stream=None):
        """The ticks' meshes (points: their vertices alone) drawn from the virtual cameras intr / wt (7 / 12 floats per view), each
        width x height.  Returns (depth int16-bit-pattern [T, V, h, w], rgb uint8 [T, V, h, w, 3]), both prefilled with SENTINEL."""
        n_views = np.asarray(intr).size // 7
        depth = torch.full((self.n_ticks, n_views, height, width), SENTINEL, dtype=torch.int16, device=self.device)
        rgb = torch.full((self.n_ticks, n_views, height, width, 3), SENTINEL % 256, dtype=torch.uint8, device=self.device)
        self.plan.render_views(intr, wt, width, height, self.vertices.data_ptr(), self.offsets.data_ptr(),
                               0 if points else self.triangles.data_ptr(), 0 if points else self.tri_offsets.data_ptr(), depth.data_ptr(),
                               rgb.data_ptr(), _stream_handle(stream))
        return depth, rgb

    def simplify(self, cell, points=False, stream=None):
        """Mesh level of detail: the ticks' meshes (points: their vertices alone) clustered on a grid of edge `cell`.  Returns fresh tensors
        (vertices uint8 [T, capacity, 16], offsets int32 [T, N+1], triangles int32 [T, 2*capacity, 3] or None, tri_offsets or None, remap
        int32 [T, capacity]); the offset tables are prefilled with SENTINEL."""
        vertices = torch.zeros_like(self.vertices)
        offsets = torch.full_like(self.offsets, SENTINEL)
        triangles = None if points else torch.zeros_like(self.triangles)
        tri_offsets = None if points else torch.full_like(self.tri_offsets, SENTINEL)
        remap = torch.zeros((self.n_ticks, self.capacity), dtype=torch.int32, device=self.device)
        self.plan.simplify(cell, self.vertices.data_ptr(), self.offsets.data_ptr(), 0 if points else self.triangles.data_ptr(),
                           0 if points else self.tri_offsets.data_ptr(), vertices.data_ptr(), offsets.data_ptr(),
                           0 if points else triangles.data_ptr(), 0 if points else tri_offsets.data_ptr(), remap.data_ptr(),
                           _stream_handle(stream))
        return vertices, offsets, triangles, tri_offsets, remap

    def fragments(self, min_vertices, stream=None):
        """Fragment filter: the connected components of fewer than `min_vertices` vertices of the ticks' meshes dropped.  Returns fresh
        tensors (vertices uint8 [T, capacity, 16], offsets int32 [T, N+1], triangles int32 [T, 2*capacity, 3], tri_offsets, remap int32
        [T, capacity], labels int32 [T, capacity]); the offset tables are prefilled with SENTINEL."""
        vertices = torch.zeros_like(self.vertices)
        offsets = torch.full_like(self.offsets, SENTINEL)
        triangles = torch.zeros_like(self.triangles)
        tri_offsets = torch.full_like(self.tri_offsets, SENTINEL)
        remap = torch.zeros((self.n_ticks, self.capacity), dtype=torch.int32, device=self.device)
        labels = torch.zeros((self.n_ticks, self.capacity), dtype=torch.int32, device=self.device)
        self.plan.fragments(min_vertices, self.vertices.data_ptr(), self.offsets.data_ptr(), self.triangles.data_ptr(),
                            self.tri_offsets.data_ptr(), vertices.data_ptr(), offsets.data_ptr(), triangles.data_ptr(), tri_offsets.data_ptr(),
                            remap.data_ptr(), labels.data_ptr(), _stream_handle(stream))
        return vertices, offsets, triangles, tri_offsets, remap, labels

    def normals(self, vertices=None, offsets=None, triangles=None, tri_offsets=None, stream=None):
        """Vertex normals of the ticks' meshes -- the batch's own, or the four tensors handed in (simplify()'s first four outputs, say).
        Returns float32 [T, capacity, 3], the batch's own tensor (allocated by the first call with every byte SENTINEL % 256, written again
        by every call): a tick's normals lie at its vertices' indices, nothing behind its nVertices is written."""
        if self._normals is None:
            self._normals = torch.full((self.n_ticks, self.capacity, 12), SENTINEL % 256, dtype=torch.uint8, device=self.device).view(torch.float32)
        self.plan.normals((self.vertices if vertices is None else vertices).data_ptr(), (self.offsets if offsets is None else offsets).data_ptr(),
                          (self.triangles if triangles is None else triangles).data_ptr(),
                          (self.tri_offsets if tri_offsets is None else tri_offsets).data_ptr(), self._normals.data_ptr(), _stream_handle(stream))
        return self._normals

    def smooth(self, iterations, lam, mu, pin_boundary=True, vertices=None, offsets=None, triangles=None, tri_offsets=None, stream=None):
        """Taubin lambda|mu smoothing of the ticks' meshes -- the batch's own, or the four tensors handed in (fragments()'s first four
        outputs, say).  Returns uint8 [T, capacity, 16], the batch's own tensor (allocated by the first call with every byte SENTINEL %
        256, written again by every call): the first nVertices records of a tick are its moved vertices, nothing behind them is written;
        offsets and triangles stay the input's."""
        if self._smoothed is None:
            self._smoothed = torch.full((self.n_ticks, self.capacity, 16), SENTINEL % 256, dtype=torch.uint8, device=self.device)
        self.plan.smooth(iterations, lam, mu, pin_boundary, (self.vertices if vertices is None else vertices).data_ptr(),
                         (self.offsets if offsets is None else offsets).data_ptr(),
                         (self.triangles if triangles is None else triangles).data_ptr(),
                         (self.tri_offsets if tri_offsets is None else tri_offsets).data_ptr(), self._smoothed.data_ptr(), _stream_handle(stream))
        return self._smoothed

    def refine(self, tick, n_refine_iters=2, n_icp_iters=10, world_R=None, world_t=None, camera_R=None, camera_t=None, clouds_out=None,
               stream=None):
        """The refine pass (native.refine_vertices) on tick `tick`'s merged cloud where it lies; clouds_out: a float32 tensor with room for
        the tick's nVertices x 3 refined points.  Synchronises the stream; returns what native.refine_vertices returns."""
        return native.refine_vertices(self.device.index, self.n_maps, self.vertices[tick].data_ptr(), self.offsets[tick].data_ptr(),
                                      n_refine_iters, n_icp_iters, world_R, world_t, camera_R, camera_t,
                                      None if clouds_out is None else clouds_out.data_ptr(), _stream_handle(stream))

    def refine_plane(self, tick, normals=None, n_refine_iters=2, n_icp_iters=10, world_R=None, world_t=None, camera_R=None, camera_t=None,
                     clouds_out=None, stream=None):
        """refine() with the point-to-plane residual (native.refine_vertices_plane).  normals: what normals() returned for the batch as it
        is now (float32 [T, capacity, 3]); None: the tensor normals() last returned."""
        normals = self._normals if normals is None else normals
        assert normals is not None, "refine_plane needs the ticks' normals: call normals() first"
        return native.refine_vertices_plane(self.device.index, self.n_maps, self.vertices[tick].data_ptr(), normals[tick].data_ptr(),
                                            self.offsets[tick].data_ptr(), n_refine_iters, n_icp_iters, world_R, world_t, camera_R, camera_t,
                                            None if clouds_out is None else clouds_out.data_ptr(), _stream_handle(stream))

    # ---- host views (each synchronises the device first) ----

    def host_offsets(self):
        """offsets [T, N+1] as a numpy array."""
        torch.cuda.synchronize(self.device)
        return self.offsets.cpu().numpy()

    def host_tri_offsets(self):
        torch.cuda.synchronize(self.device)
        return self.tri_offsets.cpu().numpy()

    def tick_bytes(self, k):
        """Host copy of tick k's merged cloud as uint8 [nVertices, 16]."""
        torch.cuda.synchronize(self.device)
        return self.vertices[k, :int(self.offsets[k, -1])].cpu().numpy()

    def tick_cloud(self, k):
        """Host copy of tick k's merged cloud as a VERTEX_DTYPE array, and its offsets."""
        return self.tick_bytes(k).view(native.VERTEX_DTYPE).reshape(-1), self.offsets[k].cpu().numpy()

    def tick_triangles(self, k):
        """Host copy of tick k's triangles int32 [nTriangles, 3], cut at tri_offsets[k, -1]."""
        torch.cuda.synchronize(self.device)
        return self.triangles[k, :int(self.tri_offsets[k, -1])].cpu().numpy()

    def close(self):
        self.plan.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def stack_rigs(rigs, n_ticks=None):
    """Rigs (synth.Rig) -> (depth int16 [T, P], rgb uint8 [T, 3P]) as numpy arrays; tick k is rigs[k % len(rigs)], T = len(rigs) unless given."""
    T = len(rigs) if n_ticks is None else n_ticks
    return (np.stack([np.ascontiguousarray(rigs[k % len(rigs)].depth_maps).view(np.int16) for k in range(T)]),
            np.stack([np.ascontiguousarray(rigs[k % len(rigs)].depth_colors) for k in range(T)]))


def upload_rigs(rigs, n_ticks=None, device=None):
    """stack_rigs() on the GPU."""
    d, c = stack_rigs(rigs, n_ticks)
    return torch.from_numpy(d).to(_device(device)), torch.from_numpy(c).to(_device(device))


def upload_rig(rig, n_ticks=1, device=None):
    """One rig, the same tick replicated n_ticks times."""
    return upload_rigs([rig], n_ticks, device)
