"""tests/oracle_backend.py -- the CPU oracle dressed in the `HipRaster` interface.

Lets the `-m "not gpu"` suite drive the product's HOST logic (generators, batching, API shapes, error behaviour of
geograypher_amd.meshes) without a GPU.  Test-only: nothing under geograypher_amd/ imports this.
"""
import numpy as np
import torch

from oracle import oracle_c, oracle_np, oracle_resize, oracle_warp


class OracleBackend:
    device = torch.device("cpu")

    def __init__(self):
        self.verts = None
        self.faces = None
        self.n_faces = 0
        self.uploads = 0
        self.vertex_order = "r1"

    def set_vertex_order(self, name):
        if name not in ("r1", "gl"):
            raise ValueError(name)
        self.vertex_order = name

    def _dev(self, array, dtype):
        if isinstance(array, torch.Tensor):
            return array.to(dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(array)).to(dtype=dtype).contiguous()

    def upload_mesh(self, verts, faces):
        self.verts = np.ascontiguousarray(np.asarray(verts), dtype=np.float32)
        self.faces = np.ascontiguousarray(np.asarray(faces), dtype=np.int32)
        if self.faces.min() < 0 or self.faces.max() >= self.verts.shape[0]:
            raise IndexError("face index outside [0, V)")
        self.n_faces = self.faces.shape[0]
        self.uploads += 1

    def raster_face_ids(self, cams, h, w, out=None, want_depth=False, check=True):
        cams = np.asarray(cams, dtype=np.float32).reshape(-1, 16)
        if self.vertex_order == "gl":
            ids = np.stack([oracle_c.raster(self.verts, self.faces, cams[v], h, w, vertex_order="gl") for v in range(cams.shape[0])])
        else:
            ids, _ = oracle_c.raster_views(self.verts, self.faces, cams, h, w, n_threads=1)
        return torch.from_numpy(ids)

    def gather_texture(self, ids, face_texture):
        ids = np.asarray(ids)
        tex = np.asarray(face_texture, dtype=np.float64)
        flat = oracle_np.render_flat_gather(ids.reshape(-1, 1).astype(np.int64), tex)
        return torch.from_numpy(flat.reshape(ids.shape + (tex.shape[1],)))

    def gather_texture_u8(self, ids, face_texture, null_value=0):
        f64 = self.gather_texture(ids, face_texture).numpy()
        with np.errstate(invalid="ignore"):
            bad = (f64 < 0) | (f64 > 255) | ~np.isfinite(f64)
        f64[bad] = null_value
        return torch.from_numpy(f64.astype(np.uint8))

    def project_index_pairs(self, ids, img, n_classes, counts, neg1_is_last_face=True):
        ids = np.asarray(ids)
        img = np.asarray(img)
        if ids.ndim == 2:
            ids, img = ids[None], img[None]
        keys = []
        for k in range(ids.shape[0]):
            proj = oracle_np.project_image(ids[k].astype(np.int64), img[k], self.n_faces,
                                           neg1_is_last_face=neg1_is_last_face)
            inds = np.nonzero(np.isfinite(proj[:, 0]))[0]
            counts += torch.from_numpy(np.bincount(inds, minlength=self.n_faces).astype(np.int32))
            cls = proj[inds, 0].astype(np.int64)
            if cls.size and (cls.min() < 0 or cls.max() >= n_classes):
                raise IndexError("class index out of range")
            keys.append(inds.astype(np.int64) * n_classes + cls)
        keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
        uniq, mult = np.unique(keys, return_counts=True)
        return uniq, mult.astype(np.int64)

    def new_pair_accumulator(self, n_classes, counts, neg1_is_last_face=True):
        backend = self

        class _Acc:
            def __init__(self):
                self.parts = []

            def add(self, ids, img):
                self.parts.append(backend.project_index_pairs(ids, np.asarray(img, dtype=np.float64), n_classes, counts,
                                                              neg1_is_last_face=neg1_is_last_face))

            def finish(self):
                if not self.parts:
                    return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
                keys = np.concatenate([p[0] for p in self.parts])
                mult = np.concatenate([p[1] for p in self.parts])
                uniq, inv = np.unique(keys, return_inverse=True)
                return uniq, np.bincount(inv, weights=mult, minlength=uniq.size).astype(np.int64)

        return _Acc()

    def new_vote_buffers(self, C):
        return torch.zeros((self.n_faces, C), dtype=torch.int32), torch.zeros((self.n_faces,), dtype=torch.int32)

    def project_labels(self, ids, labels, C, votes, counts, neg1_is_last_face=True):
        ids = np.asarray(ids)
        labels = np.asarray(labels)
        if ids.ndim == 2:
            ids, labels = ids[None], labels[None]
        v = votes.numpy().view(np.uint32)
        c = counts.numpy().view(np.uint32)
        for k in range(ids.shape[0]):
            oracle_c.project_labels(ids[k], labels[k], self.n_faces, C, v, c, neg1_is_last_face)

    def raster_project_labels(self, cams, labels, C, votes, counts, ids_out=None, neg1_is_last_face=True, check=True):
        labels = np.asarray(labels)
        ids = self.raster_face_ids(cams, labels.shape[1], labels.shape[2])
        self.project_labels(ids, labels, C, votes, counts, neg1_is_last_face=neg1_is_last_face)
        return ids

    def project_view(self, ids, img, neg1_is_last_face=True):
        tex = oracle_np.project_image(np.asarray(ids).astype(np.int64), np.asarray(img), self.n_faces,
                                      neg1_is_last_face=neg1_is_last_face)
        return torch.from_numpy(tex)

    def project_values(self, ids, img, sums, counts, neg1_is_last_face=True):
        ids = np.asarray(ids)
        img = np.asarray(img)
        if ids.ndim == 2:
            ids, img = ids[None], img[None]
        for k in range(ids.shape[0]):
            proj = oracle_np.project_image(ids[k].astype(np.int64), img[k], self.n_faces,
                                           neg1_is_last_face=neg1_is_last_face)
            # np.nansum([summed, projection], axis=0) (meshes.py:2060-2062): a NaN of the running sum is dropped like one of the projection
            s_np = sums.numpy()
            with np.errstate(invalid="ignore"):  # inf - inf
                s_np[...] = np.where(np.isnan(s_np), 0.0, s_np) + np.where(np.isnan(proj), 0.0, proj)
            counts += torch.from_numpy(np.any(np.isfinite(proj), axis=1).astype(np.int32))

    def finalize_votes(self, votes, counts):
        v = votes.numpy().view(np.uint32).astype(np.float64)
        c = counts.numpy().view(np.uint32).astype(np.float64)
        summed = v.copy()
        summed[c == 0] = np.nan
        with np.errstate(divide="ignore", invalid="ignore"):
            avg = summed / c[:, None]
        return torch.from_numpy(avg), torch.from_numpy(summed), torch.from_numpy(c)

    def finalize_sums(self, sums, counts):
        s = sums.numpy().copy()
        c = counts.numpy().astype(np.float64)
        s[c == 0] = np.nan
        with np.errstate(divide="ignore", invalid="ignore"):
            avg = s / c[:, None]
        return torch.from_numpy(avg), torch.from_numpy(s), torch.from_numpy(c)

    def resize_image(self, image, out_hw=None, divide_by_255=None):
        img = image.numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
        if divide_by_255 is None:
            divide_by_255 = img.dtype == np.uint8
        img = img / 255.0 if divide_by_255 else img.astype(np.float64)
        if out_hw is not None and tuple(out_hw) != img.shape[:2]:
            img = oracle_resize.resize_antialias(img, out_hw)
        return torch.from_numpy(np.ascontiguousarray(img))

    def upload_map(self, inverse_map):
        return torch.from_numpy(np.ascontiguousarray(inverse_map, dtype=np.float64))

    def invert_distortion(self, params, h, w, image_scale=1.0, max_iters=12, fill=-1.0):
        return torch.from_numpy(oracle_warp.newton_inverse_map(dict(params), h, w, image_scale, fill=fill))

    def warp_image(self, input_image, map_t, order=1, fill_value=0.0, reference_float_roundtrip=False):
        img = np.asarray(input_image)
        if reference_float_roundtrip:
            # the combinations HipRaster.warp_image reproduces, and its refusal of the others (the constant shortcut first)
            lo, hi = min(float(np.min(img)), float(fill_value)), max(float(np.max(img)), float(fill_value))
            small_int = (np.issubdtype(img.dtype, np.integer) or img.dtype == bool) and -2**31 <= lo and hi < 2**31 \
                and float(fill_value) == int(fill_value)
            if hi - lo != 0 and not (small_int and order == 0):
                raise NotImplementedError("reference_float_roundtrip=True is reproduced only for order 0 on integer images "
                                          "within the int32 range with an integer fill value")
            return oracle_warp.flexible_inputs_warp_reference(img, map_t.numpy(), order, fill_value)
        # warp_total: warp_exact (scipy) restated so that NaN / infinite coordinates read the fill value, as the kernels do
        return oracle_warp.warp_total(img, map_t.numpy(), order, fill_value)

    def argmax_nonzero(self, array):
        return torch.from_numpy(oracle_np.find_argmax_nonzero_value(np.asarray(array)))
