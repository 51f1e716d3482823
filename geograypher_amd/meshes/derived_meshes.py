"""Derived mesh classes of the reference, on the GPU path.

Mirror of geograypher/meshes/derived_meshes.py for the two variants whose work is the projection path:

* `TexturedPhotogrammetryMeshChunked` (derived_meshes.py:23-317) exists in the reference because the VTK render cost
  grows with the mesh: it clusters the cameras (KMeans), crops a sub-mesh per cluster and renders chunk by chunk.
  Here every view is frustum-culled on the device per 256-face block and binned per tile, so the whole mesh is
  rendered at once and the class only keeps the reference's constructor/method signatures: results are those of the
  un-chunked class (a superset of what a 125 m-buffered chunk can see).
* `TexturedPhotogrammetryMeshIndexPredictions` (derived_meshes.py:414-550): aggregation of single-channel class-index
  images with many classes into scipy CSR arrays; the per-view projection, pair emission, radix sort and
  run-length count run on the device (`gr_project_index_pairs`, `gr_count_pairs`).  Where the camera set's segmentor
  describes its label images as rectangles (detections, image IDs: `get_label_rectangles`), no label image is built at
  all: the label of a face's winning pixel is looked up in the view's rectangle table (`gr_project_rect_pairs`).  Where it
  describes them as polygon rings (region detections: `get_label_regions`), the (h, w, C) multi-hot mask is never built
  either: the winning pixel is tested against the view's rings and is one observation of every class that contains it
  (`gr_project_polygon_pairs`).
"""
import typing

import numpy as np

from geograypher_amd.cameras.cameras import PhotogrammetryCamera, PhotogrammetryCameraSet
from geograypher_amd.meshes.meshes import TexturedPhotogrammetryMesh, _batched_views, _torch, tqdm

CHUNKED_MESH_BUFFER_DIST_METERS = 125  # geograypher/constants.py:130


class TexturedPhotogrammetryMeshChunked(TexturedPhotogrammetryMesh):
    """Drop-in for the reference's chunked class; `n_clusters`, `buffer_dist_meters` and `vis_clusters` are accepted and
    ignored (the GPU path needs no chunking)."""

    def _say_unchunked(self, what, n_clusters, buffer_dist_meters, vis_clusters):
        """One log line per call: the chunking arguments are accepted for signature compatibility and have no effect."""
        self.logger.info(
            f"{what}: n_clusters={n_clusters}, buffer_dist_meters={buffer_dist_meters}, vis_clusters={vis_clusters} are "
            "ignored -- the GPU path culls and bins the whole mesh per view, no camera clustering or sub-mesh cropping; "
            "views are processed in CAMERA order (the reference goes cluster by cluster, derived_meshes.py:206, 281)"
        )

    def render_flat(self, cameras, batch_size: int = 1, render_img_scale: float = 1, n_clusters: int = 8,
                    buffer_dist_meters: float = CHUNKED_MESH_BUFFER_DIST_METERS, vis_clusters: bool = False,
                    **pix2face_kwargs):
        """reference: derived_meshes.py:153-220.  NOTE: the reference yields the renders cluster by cluster, i.e. in
        KMeans cluster order; here they come in camera order."""
        self._say_unchunked("render_flat", n_clusters, buffer_dist_meters, vis_clusters)
        yield from super().render_flat(cameras, batch_size=batch_size, render_img_scale=render_img_scale,
                                       **pix2face_kwargs)

    def aggregate_projected_images(self, cameras, batch_size: int = 1, aggregate_img_scale: float = 1,
                                   n_clusters: int = 8, buffer_dist_meters: float = CHUNKED_MESH_BUFFER_DIST_METERS,
                                   vis_clusters: bool = False, **kwargs):
        """reference: derived_meshes.py:222-317 (same return structure as the base class)."""
        self._say_unchunked("aggregate_projected_images", n_clusters, buffer_dist_meters, vis_clusters)
        return super().aggregate_projected_images(cameras, batch_size=batch_size,
                                                  aggregate_img_scale=aggregate_img_scale, **kwargs)

    def save_renders(self, camera_set, *args, n_clusters: int = 8,
                     buffer_dist_meters: float = CHUNKED_MESH_BUFFER_DIST_METERS, vis_clusters: bool = False, **kwargs):
        """The base class's `save_renders`; the chunking arguments the reference's forwards to its chunked `render_flat`
        (meshes.py:2300-2305 -> derived_meshes.py:153-220) are accepted and ignored."""
        self._say_unchunked("save_renders", n_clusters, buffer_dist_meters, vis_clusters)
        return super().save_renders(camera_set, *args, **kwargs)

    def label_polygons(self, face_labels, polygons, face_weighting=None, sjoin_overlay: bool = True,
                       return_class_labels: bool = True, unknown_class_label: str = "unknown",
                       buffer_dist_meters: float = 2.0, n_polygons_per_cluster: int = 1000, *, points_in_polygon_CRS=None):
        """reference: derived_meshes.py:319-411, which clusters the polygons (KMeans) to keep gpd.overlay tractable; here every
        face meets every polygon's box in one kernel, so `n_polygons_per_cluster` is accepted and ignored."""
        self.logger.info(f"label_polygons: n_polygons_per_cluster={n_polygons_per_cluster} is ignored -- one kernel meets every "
                         "face with every polygon's box, no polygon clustering")
        return super().label_polygons(face_labels, polygons, face_weighting=face_weighting, sjoin_overlay=sjoin_overlay,
                                      return_class_labels=return_class_labels, unknown_class_label=unknown_class_label,
                                      buffer_dist_meters=buffer_dist_meters, points_in_polygon_CRS=points_in_polygon_CRS)

class TexturedPhotogrammetryMeshIndexPredictions(TexturedPhotogrammetryMesh):
    def aggregate_projected_images(
        self,
        cameras: typing.Union[PhotogrammetryCamera, PhotogrammetryCameraSet],
        n_classes: int,
        batch_size: int = 1,
        aggregate_img_scale: float = 1,
        return_all: bool = False,
        **kwargs,
    ):
        """Sparse aggregation of class-index images (reference: derived_meshes.py:415-550).

        Every image is (h, w) or (h, w, 1) float with NaN where nothing was predicted and a class index elsewhere.
        Returns `(average (F, n_classes) scipy CSR, {"projection_counts": CSR (F,1) int, "summed_projections": CSR
        (F, n_classes) int[, "all_projections"]})` exactly like the reference.
        """
        from scipy.sparse import csr_array

        if len(cameras) == 0 or batch_size > len(cameras):
            raise IndexError("list index out of range")
        torch = _torch()
        n_faces = self.faces.shape[0]
        kwargs.pop("check_null_image", None)
        all_projections = [] if return_all else None
        backend = self.backend
        counts = torch.zeros((n_faces,), dtype=torch.int32, device=backend.device)
        # the (face, class) pair keys of all views stay on the device; ONE sort + run-length count at the end
        acc = backend.new_pair_accumulator(n_classes, counts, neg1_is_last_face=self.neg1_is_last_face)
        batch_stop, view_inds = _batched_views(len(cameras), batch_size)
        # a camera set whose segmentor describes every used view as rectangles, or as polygon rings, is aggregated from those
        # tables: no label image is loaded or built
        tables = None
        for supplier, consumer, add_tables in (("get_label_rectangles", "add_rects", self._add_rectangle_tables),
                                               ("get_label_regions", "add_polygons", self._add_region_tables)):
            if tables is None and not return_all and hasattr(acc, consumer) and hasattr(cameras, supplier):
                tables = [getattr(cameras, supplier)(i, aggregate_img_scale) for i in view_inds]
                if any(t is None for t in tables):
                    tables = None
                else:
                    self._add_table_pairs(acc, add_tables, cameras, tables, batch_size, batch_stop, aggregate_img_scale, kwargs)
        gen = () if tables is not None else self._iter_view_inputs(backend, cameras, batch_size, aggregate_img_scale, True, kwargs)
        for _, ids, img, n_channels in tqdm(gen, total=len(cameras), desc="Aggregating projected viewpoints"):
            if return_all:
                if img is None:
                    all_projections.append(np.full((n_faces, n_channels), fill_value=np.nan))
                else:
                    all_projections.append(
                        backend.project_view(ids, img, neg1_is_last_face=self.neg1_is_last_face).cpu().numpy()
                    )
            if img is None:  # null image: nothing to project (check_null_image=True, derived_meshes.py:465)
                continue
            if img.shape[-1] != 1:
                raise ValueError("index predictions must be single-channel images")
            acc.add(ids, img[..., 0])
        uniq, mult = acc.finish()
        summed_vals = mult.astype(int)
        rows, cols = uniq // n_classes, uniq % n_classes
        summed_projections = csr_array((summed_vals, (rows, cols)), shape=(n_faces, n_classes), dtype=int)
        cnt = counts.cpu().numpy().astype(int)
        seen = np.nonzero(cnt)[0]
        projection_counts = csr_array((cnt[seen], (seen, np.zeros_like(seen))), shape=(n_faces, 1), dtype=int)
        info = {"projection_counts": projection_counts, "summed_projections": summed_projections}
        if return_all:
            info["all_projections"] = all_projections
        reciprocal = csr_array(
            (np.reciprocal(projection_counts.data.astype(float)), projection_counts.indices, projection_counts.indptr),
            shape=projection_counts.shape,
        )
        average_projections = summed_projections.multiply(reciprocal)
        return average_projections, info

    def select_covering_cameras(self, cameras, min_observations_to_be_included=1, prune: bool = True,
                                aggregate_img_scale: float = 1, **kwargs):
        """A small set of cameras that together see every face the set sees -- both halves of annotation_image_selection
        (reference: entrypoints/annotation_image_selection.py:99-117, 142-174): the face x view visibility matrix from
        `aggregate_projected_images` with every view labelled by its own index (`ImageIDSegmentor`; `cameras` is wrapped unless it
        is a `SegmentorPhotogrammetryCameraSet` already), then `select_covering_views` on the device.
        Returns (mask (len(cameras),) bool, the selection record, summed_projections (F, len(cameras)) CSR); `kwargs` go to
        `aggregate_projected_images`."""
        from geograypher_amd.cameras.segmentor import SegmentorPhotogrammetryCameraSet
        from geograypher_amd.predictors.derived_segmentors import ImageIDSegmentor
        from geograypher_amd.utils.numeric import select_covering_views

        if not isinstance(cameras, SegmentorPhotogrammetryCameraSet):
            segmentor = ImageIDSegmentor(image_filenames=cameras.get_image_filename(index=None, absolute=True))
            cameras = SegmentorPhotogrammetryCameraSet(base_camera_set=cameras, segmentor=segmentor)
        _, info = self.aggregate_projected_images(cameras, n_classes=len(cameras), aggregate_img_scale=aggregate_img_scale, **kwargs)
        summed_projections = info["summed_projections"]
        record = select_covering_views(summed_projections, min_observations_to_be_included=min_observations_to_be_included,
                                       prune=prune, backend=self.backend)
        return record["selected"], record, summed_projections

    def _add_table_pairs(self, acc, add_tables, cameras, tables, batch_size, batch_stop, aggregate_img_scale, pix2face_kwargs):
        """The table paths of `aggregate_projected_images` (label rectangles, polygon rings): ids come from `_driver_ids` exactly
        as on the image path (same batches, mesh, distortion and keywords); `add_tables(acc, ids, [table of each view])` sends
        the batch's tables to the device, where the label(s) of each face's winning pixel are looked up."""
        backend, mesh = self.backend, self.get_mesh_in_cameras_coords(cameras)
        for batch_start in tqdm(range(0, batch_stop, batch_size), desc="Aggregating projected viewpoints"):
            batch_cameras = cameras.get_subset_cameras(list(range(batch_start, batch_start + batch_size)))
            ids = self._driver_ids(backend, batch_cameras, mesh, aggregate_img_scale, pix2face_kwargs)
            batch = tables[batch_start:batch_start + batch_size]
            for _, hw in batch:
                if tuple(hw) != tuple(ids.shape[1:]):
                    raise ValueError(
                        f"ids {tuple(ids.shape[1:])} and index image {tuple(hw)} differ in shape"
                    )
            add_tables(acc, ids, [table for table, _ in batch])

    @staticmethod
    def _add_rectangle_tables(acc, ids, batch):
        """One (R, 5) rectangle table per view -> one `add_rects`."""
        offsets = np.zeros(len(batch) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([rects.shape[0] for rects in batch])
        acc.add_rects(ids, np.concatenate(batch), offsets)

    @staticmethod
    def _add_region_tables(acc, ids, batch):
        """One (boxes, vert_offsets, verts) ring table per view -> one `add_polygons`."""
        poly_offsets = np.zeros(len(batch) + 1, dtype=np.int64)
        poly_offsets[1:] = np.cumsum([boxes.shape[0] for boxes, _, _ in batch])
        vert_base = np.concatenate([[0], np.cumsum([verts.shape[0] for _, _, verts in batch])]).astype(np.int64)
        vert_offsets = np.concatenate([[0]] + [np.asarray(vo, dtype=np.int64)[1:] + vert_base[k]
                                               for k, (_, vo, _) in enumerate(batch)])
        acc.add_polygons(ids, np.concatenate([np.asarray(boxes).reshape(-1, 5) for boxes, _, _ in batch]), vert_offsets,
                         np.concatenate([np.asarray(verts, dtype=np.float64).reshape(-1, 2) for _, _, verts in batch]),
                         poly_offsets)
