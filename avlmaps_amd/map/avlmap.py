"""AVLMap facade (avlmaps/map/avlmap.py:18-163): the VLMap sub-map with create_map / load_map / index_object, and the area, sound
and image goal queries.

The four queries end in a per-voxel heat on the GPU.  For area and sound the per-pose / per-segment distance transforms of
upstream (one full-grid scipy EDT each) are one kernel that builds the 2-D field (csrc/avl_field2d.hip), and the Python loop over
occupied_ids is one lift kernel reading the map's device-resident grid_pos.  The models around them (CLIP ViT-L/14 frame
embeddings, AudioCLIP, HLoc) are pluggable, and whatever a query needs that is not loaded or attached raises MissingSubMap, a
NotImplementedError that says what to provide.

Departures from the reference, all where upstream fails or depends on an online service:
  * category lookups go through utils/index_utils.find_similar_category_id (KeyError when nothing matches), not an LLM;
  * a sound location outside the grid raises ValueError (upstream: IndexError, or a silently wrapped negative index);
  * a degenerate min-max normalisation (max == min, of the scores or of the 2-D field) raises ValueError (upstream: NaN
    everywhere), as index_object raises where upstream's argmin does;
  * decay_rate must be finite and >= 0 for area and sound (ValueError)."""
from __future__ import annotations

from pathlib import Path
from typing import List

import numpy as np

from ..utils.visualize_utils import get_heatmap_from_mask_3d
from .map import cfg_get
from .vlmap import VLMap


class MissingSubMap(NotImplementedError):
    """An AVLMap query whose sub-map (area / sound) or image localiser has not been loaded or attached."""


def _opt(cfg, key, default=None):
    try:
        return cfg_get(cfg, key)
    except (KeyError, AttributeError):
        return default


class AVLMap:
    def __init__(self, config, data_dir: str = "", area_text_model=None, audio_text_model=None, localizer=None, audio_encoder=None):
        """area_text_model: the CLIP ViT-L/14 text tower (or a stand-in) of the area queries, loaded on demand when None;
        audio_text_model: AudioCLIP's text side (map/sound_map.py); localizer: the image localiser (map/visual_map.py);
        audio_encoder: AudioCLIP's audio head or a stand-in, for create_map's sound map and get_pos_with_audio."""
        from .area_map import AreaMap
        from .visual_map import VisualMap
        self.config = config
        self.vlmap = VLMap(cfg_get(config, "map_config"), data_dir=data_dir)
        self.area_map = AreaMap(clip_model=area_text_model)
        self.visual_map = VisualMap(cfg_get(config, "map_config"), data_dir, localizer=localizer)
        self.sound_map = None
        sound_cfg, sound_params = _opt(config, "sound_config"), _opt(config, "sound_data_collect_params")
        if sound_cfg is not None and sound_params is not None:
            from .sound_map import SoundMap
            self.sound_map = SoundMap(data_dir, sound_cfg, sound_params, is_ambiguous=False, is_real=False,
                                      audio_text_model=audio_text_model, audio_encoder=audio_encoder)
        self._area_loaded = self._sound_loaded = False
        self._dataloader = None
        self._area_cells = self._sound_cells = None
        self._rooms = self._room_names = None

    # ------------------------------------------------------------------ build / load
    def create_map(self, data_dir, feat_extractor=None, area_encoder=None, audio_encoder=None, area_batch_encoder=None) -> bool:
        """Reference: avlmap.py:38-46.  area_encoder(rgb) -> (768,): also build the area map (area_map/clip_sparse_map.h5df), frame by
        frame; area_batch_encoder((B, 3, n_px, n_px) device tensor) -> (B, 768): build it in batches preprocessed on the GPU.
        audio_encoder(batch (B, 5 * sample_rate)) -> (B, D): also build the sound map (audio_video/audio_data_<level>.pkl) when the
        configuration has a sound part and the scene an audio_video directory."""
        self.vlmap.create_map(data_dir, feat_extractor=feat_extractor)
        if area_encoder is not None:
            self.area_map.create_map(data_dir, image_encoder=area_encoder)
        elif area_batch_encoder is not None:
            self.area_map.create_map(data_dir, batch_encoder=area_batch_encoder)
        if audio_encoder is not None:
            if self.sound_map is None:
                raise MissingSubMap("AVLMap.create_map(audio_encoder=...) needs sound_config and sound_data_collect_params in the "
                                    "configuration")
            self.sound_map.create_sound_map(data_dir, audio_encoder=audio_encoder)
        return True

    def load_map(self, data_dir: str) -> bool:
        """Reference: avlmap.py:48-54.  The area and sound maps are loaded when their files exist; the poses they refer to are
        converted to map cells once here, so that a query costs the text tower, one matmul, the field and the lift."""
        if not self.vlmap.load_map(data_dir):
            return False
        from .area_map import AreaMap
        self._dataloader = None
        self._area_cells = self._sound_cells = None
        self._rooms = self._room_names = None
        self._area_loaded = AreaMap.map_exists(data_dir) and self.area_map.load_map(data_dir)
        self._sound_loaded = False
        if self.sound_map is not None and self.sound_map.sound_map_path(data_dir).exists():
            self.sound_map.load_sound_map(data_dir)
            self._sound_loaded = True
        return True

    @property
    def dataloader(self):
        """VLMapsDataloaderHabitat of the loaded map (avlmap.py:53)"""
        if self._dataloader is None:
            from ..dataloader.habitat_dataloader import VLMapsDataloaderHabitat
            vm = self.vlmap
            self._dataloader = VLMapsDataloaderHabitat(vm.data_dir, cfg_get(self.config, "map_config"), vm)
        return self._dataloader

    @dataloader.setter
    def dataloader(self, value):
        self._dataloader = value

    def index_object(self, object_name: str, init_categories: List[str] = None, decay_rate: float = 0.1) -> np.ndarray:
        """(N,) float32 heat.  Reference: avlmap.py:67-76."""
        cs = cfg_get(cfg_get(self.config, "params"), "cs")
        if init_categories is not None:
            self.vlmap.init_categories(init_categories[1:-1])
            mask = self.vlmap.index_map(object_name, with_init_cat=True)
            return get_heatmap_from_mask_3d(self.vlmap.grid_pos, mask, cell_size=cs, decay_rate=decay_rate)
        # query -> argmax -> mask -> heat without leaving the GPU: only the (N,) float32 heat comes back
        return self._object_heat(object_name, decay_rate).numpy()

    def _object_heat(self, object_name: str, decay_rate: float):
        """index_object's heat while it is still on the device: (N,) float32.  ValueError when no voxel matches."""
        from .. import ops
        cs = cfg_get(cfg_get(self.config, "params"), "cs")
        vm = self.vlmap
        q = vm._text_feats([object_name])            # cached per string: the text tower costs more than the kernels below
        feat = vm._device_feat()
        if vm._rows != (0, len(vm.grid_feat)):          # voxel rows sharded over ranks: gather the argmax, heat on the full map
            mask = vm._score(q, want_scores=False)[1] == 0
            if not mask.any():
                raise ValueError("attempt to get argmin of an empty sequence")
            return vm.heatmap_from_mask(mask.astype(np.uint8), cs, decay_rate)
        _, am, _ = ops.sim_scores(feat, q, want_scores=False, want_argmax=True, precision=vm._sim_precision)
        mask = ops.mask_from_argmax(am, 0)
        heat = vm.heatmap_from_mask(mask, cs, decay_rate)
        if vm.grid_pos.shape[0] and ops.argmax_f32(heat)[1] < 1.0:      # a target voxel has heat exactly 1
            raise ValueError("attempt to get argmin of an empty sequence")   # what np.argmin raises upstream (no voxel matched)
        return heat

    def index_object_instance(self, object_name: str, k: int, decay_rate: float = 0.1, min_voxels: int = 50,
                              connectivity: int = 26) -> np.ndarray:
        """(N,) float32 heat of ONE object: instance k of VLMap.get_instances_3d(object_name, min_voxels, connectivity), 1 on its
        voxels and decaying from them alone.  Upstream has no counterpart (avlmap.py:67-76 heats every voxel of the category).
        Needs vlmap.init_categories.  IndexError when k is not a label of the category or the instance has fewer than min_voxels
        voxels.  The heat can go into index_goal(extra=[...]) as it stands."""
        cs = cfg_get(cfg_get(self.config, "params"), "cs")
        vm = self.vlmap
        _, inst = vm._instances_3d(object_name, connectivity)
        if not 1 <= int(k) <= inst.n:
            raise IndexError(f"{object_name!r} has {inst.n} instances, asked for {k}")
        if inst.table[int(k) - 1, 0] < int(min_voxels):
            raise IndexError(f"instance {k} of {object_name!r} has {int(inst.table[int(k) - 1, 0])} voxels, fewer than min_voxels = {min_voxels}")
        return vm.heatmap_from_mask(inst.mask_of(int(k)), cs, decay_rate).numpy()

    def index_scene_object(self, label: int, decay_rate: float = 0.1, min_voxels: int = 50, connectivity: int = 26) -> np.ndarray:
        """(N,) float32 heat of ONE object of the scene: object `label` of VLMap.get_objects(min_voxels, connectivity), 1 on its voxels
        and decaying from them alone -- index_object_instance without naming the category.  Upstream has no counterpart
        (avlmap.py:67-76 heats every voxel of a category).  Needs vlmap.init_categories.  IndexError when `label` is no object of the
        scene or the object has fewer than min_voxels voxels.  The heat can go into index_goal(extra=[...]) as it stands."""
        cs = cfg_get(cfg_get(self.config, "params"), "cs")
        vm = self.vlmap
        vo = vm.get_objects(min_voxels=min_voxels, connectivity=connectivity).voxel_objects
        if not 1 <= int(label) <= vo.n:
            raise IndexError(f"the scene has {vo.n} objects, asked for {label}")
        if vo.table[int(label) - 1, 0] < int(min_voxels):
            raise IndexError(f"object {label} has {int(vo.table[int(label) - 1, 0])} voxels, fewer than min_voxels = {min_voxels}")
        return vm.heatmap_from_mask(vo.mask_of(int(label)), cs, decay_rate).numpy()

    def index_changes(self, changes, kinds=("appeared", "changed"), decay_rate: float = 0.1) -> np.ndarray:
        """(N,) float32 heat that decays from the voxels of a MapChanges (VLMap.compare) named in `kinds`: 1 on them.  This map is
        the one whose voxels the kinds lie over: "appeared", "changed" and "unseen_b" the later map B's (`other` of compare),
        "vanished", "unseen" and "changed_a" the earlier map A's; ValueError when the kinds mix the two or the voxel count is
        another map's, or when no voxel is marked.  Upstream has no counterpart.  The heat can go into index_goal(extra=[...]) as
        it stands: go and look at what changed."""
        cs = cfg_get(cfg_get(self.config, "params"), "cs")
        vm = self.vlmap
        kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
        mask = changes.mask(kinds)
        if mask.shape != (len(vm.grid_pos),):
            raise ValueError(f"index_changes: {tuple(kinds)} mark {mask.shape[0]} voxels, this map has {len(vm.grid_pos)}")
        if not mask.any():
            raise ValueError(f"index_changes: no voxel is {' or '.join(kinds)}")
        return vm.heatmap_from_mask(mask.astype(np.uint8), cs, decay_rate).numpy()

    def index_related_object(self, subject: str, relation: str, anchor: str, decay_rate: float = 0.1, radius: float = 0.25,
                             **kwargs) -> np.ndarray:
        """(N,) float32 heat of "the mug on the table": index_scene_object's heat of the subject of the FIRST hit of
        VLMap.get_scene_graph(radius, **kwargs).find(subject, relation, anchor) -- relation one of "near", "on", "under",
        "touching", the names matched against the objects' voted categories, the hits in find's documented order; kwargs are
        get_objects' min_voxels, connectivity and exclude.  LookupError when no pair of listed objects stands in that relation.
        Upstream has no counterpart.  Needs vlmap.init_categories.  The heat can go into index_goal(extra=[...]) as it stands."""
        cs = cfg_get(cfg_get(self.config, "params"), "cs")
        vm = self.vlmap
        graph = vm.get_scene_graph(radius=radius, **kwargs)
        hits = graph.find(subject, relation, anchor)
        if not hits:
            raise LookupError(f"no {subject!r} {relation} a {anchor!r} among the {len(graph.objects.objects)} listed objects "
                              f"within {graph.R} cells")
        return vm.heatmap_from_mask(graph.objects.voxel_objects.mask_of(hits[0][0].label), cs, decay_rate).numpy()

    # ------------------------------------------------------------------ area
    def _require_area(self):
        if not self._area_loaded:
            raise MissingSubMap("AVLMap.index_area needs the area map: create it with create_map(data_dir, area_encoder=...) and "
                                "load_map(data_dir) (reads area_map/clip_sparse_map.h5df)")

    def _area_field(self, area_name: str, decay_rate: float):
        from .. import ops
        self._require_area()
        scores = self.area_map.index_map(area_name, with_init_cat=False)
        lo, hi = np.min(scores), np.max(scores)
        if not hi > lo:
            raise ValueError(f"area {area_name!r}: every frame has the same score, the min-max normalisation is undefined")
        peaks = ((scores - lo) / (hi - lo)).astype(np.float64)          # float32 normalisation, as upstream (avlmap.py:81)
        if self._area_cells is None:
            cells = self.dataloader.habitat_tfs_to_cells(self.area_map.robot_pose_list)
            cells = np.clip(cells, -1, np.iinfo(np.int32).max).astype(np.int32)   # (anything negative is outside the grid alike)
            from ..device import DeviceArray
            self._area_cells = DeviceArray.from_numpy(cells)
        return ops.area_field(self._area_cells, peaks, self.vlmap.gs, decay_rate)

    @staticmethod
    def _check_bounds(gf, what):
        lo, hi = gf.bounds()
        if not hi > lo:
            raise ValueError(f"{what}: the 2-D map is constant ({lo}), its min-max normalisation is undefined")

    def index_area_2d(self, area_name: str, decay_rate: float = 0.1) -> np.ndarray:
        """(gs, gs) float64.  Reference: avlmap.py:78-98."""
        from .. import ops
        gf = self._area_field(area_name, decay_rate)
        self._check_bounds(gf, f"area {area_name!r}")
        return ops.field_normalize(gf).numpy()

    def index_area(self, area_name: str, decay_rate: float = 0.1) -> np.ndarray:
        """(N,) float32.  Reference: avlmap.py:100-109."""
        gf = self._area_field(area_name, decay_rate)
        return self._lift(gf, f"area {area_name!r}")

    def _vh(self) -> int:
        vm = self.vlmap
        return vm.occupied_ids.shape[2] if vm.occupied_ids is not None else np.iinfo(np.int32).max

    def _lift(self, gf, what):
        from .. import ops
        heat = ops.field_lift(gf, self.vlmap._device_pos(), self._vh())
        self._check_bounds(gf, what)
        return heat.numpy()

    # ------------------------------------------------------------------ rooms
    def get_rooms(self, **kwargs):
        """the Rooms of the voxel map (Map.get_rooms), kept for name_rooms and index_room until the next call with arguments"""
        if kwargs or getattr(self, "_rooms", None) is None:
            self._rooms, self._room_names = self.vlmap.get_rooms(**kwargs), None
        return self._rooms

    def _frame_cells(self) -> np.ndarray:
        """(F, 2) int32 full-map cells of the area map's frames, exactly the cells _area_field hands to the kernel"""
        cells = self.dataloader.habitat_tfs_to_cells(self.area_map.robot_pose_list)
        return np.clip(cells, -1, np.iinfo(np.int32).max).astype(np.int32)

    def name_rooms(self, names: List[str], rooms=None) -> list:
        """A name for every room: [name of room 1, .., name of room K].  A room's score for a name is the float64 mean of the area
        map's frame scores (AreaMap.index_map, as index_area reads them) over the frames whose pose cell lies in the room -- a
        sequential sum in frame order on the host; the room's name is the first maximum over `names`, None for a room without a
        frame.  rooms: a Rooms (kept for index_room), by default get_rooms().  The scores stay on self.room_scores (K, len(names))
        float64, NaN for a room without a frame."""
        self._require_area()
        names = [str(s) for s in names]
        if not names:
            raise ValueError("name_rooms needs at least one name")
        if rooms is None:
            rooms = self.get_rooms()
        self._rooms = rooms
        frame_room = np.array([rooms.room_of(cell) for cell in self._frame_cells()], dtype=np.int64)
        scores = [np.asarray(self.area_map.index_map(name, with_init_cat=False)).reshape(-1) for name in names]
        table = np.full((rooms.n, len(names)), np.nan, dtype=np.float64)
        out = []
        for k in range(1, rooms.n + 1):
            frames = np.flatnonzero(frame_room == k)
            if not len(frames):
                out.append(None)
                continue
            for q, s in enumerate(scores):
                total = 0.0
                for f in frames:                                  # frame order, one float64 addition per frame
                    total += float(s[f])
                table[k - 1, q] = total / len(frames)
            out.append(names[int(np.argmax(table[k - 1]))])
        self.room_scores, self._room_names = table, out
        return out

    def _room_ids(self, room) -> List[int]:
        rooms = self.get_rooms()
        if isinstance(room, str):
            named = getattr(self, "_room_names", None)
            if named is None:
                raise ValueError(f"room {room!r}: call name_rooms first")
            ids = [k + 1 for k, name in enumerate(named) if name == room]
            if not ids:
                raise LookupError(f"no room is named {room!r} (the names: {named})")
            return ids
        return [rooms._check(room)]

    def index_room_2d(self, room) -> np.ndarray:
        """(h, w) float64 over the obstacle crop: 1.0 on the cells of the room, 0.0 elsewhere.  room: an id, or a name that
        name_rooms gave (every room of that name)."""
        return np.isin(self.get_rooms().labels, self._room_ids(room)).astype(np.float64)

    def index_room(self, room, decay_rate: float = None) -> np.ndarray:
        """(N,) float64: 1.0 on the voxels of the room and 0.0 elsewhere (VLMap.get_voxel_rooms), a factor for index_goal:
        index_goal(obj="sofa", extra=[avl.index_room("kitchen")]) is the sofa in the kitchen.  room: an id, or a name that
        name_rooms gave (every room of that name).  decay_rate: None for the indicator; a number lets the heat decay with the
        distance from the room's voxels as index_object's does (ValueError when the room holds no voxel)."""
        inside = np.isin(self.vlmap.get_voxel_rooms(self.get_rooms()), self._room_ids(room))
        if decay_rate is None:
            return inside.astype(np.float64)
        if not inside.any():
            raise ValueError(f"room {room!r} holds no voxel")
        cs = cfg_get(cfg_get(self.config, "params"), "cs")
        return self.vlmap.heatmap_from_mask(inside.astype(np.uint8), cs, decay_rate).numpy().astype(np.float64)

    # ------------------------------------------------------------------ sound
    def _require_sound(self):
        if self.sound_map is None:
            raise MissingSubMap("AVLMap.index_sound needs sound_config and sound_data_collect_params in the config")
        if not self._sound_loaded:
            raise MissingSubMap("AVLMap.index_sound needs the sound map: load_map(data_dir) reads "
                                f"audio_video/{self.sound_map.sound_map_path('.').name}")
        if self.sound_map.aclp is None:
            raise MissingSubMap("AVLMap.index_sound needs an audio-text model: AVLMap(..., audio_text_model=...) or "
                                "sound_map.aclp = ...")

    def _sound_segments(self, sound_name: str):
        """(probabilities (S,), CSR offsets (S + 1,), cells (L, 2) int32 full-map (row, col)) of the sound segments"""
        self._require_sound()
        probabilities, locations = self.sound_map.get_distribution_and_locations(sound_name)
        if self._sound_cells is None:
            counts = np.array([len(l) for l in locations], dtype=np.int64)
            if np.any(counts == 0):
                raise ValueError("a sound segment without locations")
            pts = [np.asarray(p, dtype=np.float64).reshape(3) for l in locations for p in l]
            cells = self.dataloader.habitat_positions_to_cells(pts)
            gs = self.vlmap.gs
            if len(cells) and (cells.min() < 0 or cells.max() >= gs):
                raise ValueError(f"a sound location lies outside the {gs} x {gs} map")
            self._sound_cells = (np.concatenate([[0], np.cumsum(counts)]), cells.astype(np.int32))
        offsets, cells = self._sound_cells
        return probabilities, offsets, cells

    def _sound_field(self, sound_name: str, decay_rate: float):
        from .. import ops
        probabilities, offsets, cells = self._sound_segments(sound_name)
        return ops.sound_field(offsets, cells, probabilities, self.vlmap.gs, decay_rate)

    def index_sound_2d(self, sound_name: str, decay_rate: float = 0.01) -> np.ndarray:
        """(gs, gs) float32.  Reference: avlmap.py:111-133."""
        from .. import ops
        gf = self._sound_field(sound_name, decay_rate)
        self._check_bounds(gf, f"sound {sound_name!r}")
        return ops.field_normalize(gf).numpy()

    def _sound_travel_device(self, sound_name: str, decay_rate: float = 0.01):
        """index_sound_2d_travel's map as an (h, w) float32 DeviceArray"""
        from .. import ops
        probabilities, offsets, cells = self._sound_segments(sound_name)
        vm = self.vlmap
        r0, r1, c0, c1 = vm._crop_window()
        free = vm._travel_free()
        inside = (cells[:, 0] >= r0) & (cells[:, 0] < r1) & (cells[:, 1] >= c0) & (cells[:, 1] < c1)
        sets, peaks = [], []
        for s, p in enumerate(np.asarray(probabilities, dtype=np.float32)):
            own = cells[offsets[s]:offsets[s + 1]][inside[offsets[s]:offsets[s + 1]]]
            if len(own):                                 # a segment with no location left adds nothing
                sets.append(own - np.array([r0, c0], dtype=cells.dtype))
                peaks.append(p)
        if not sets:
            raise ValueError(f"sound {sound_name!r}: no sound location lies inside the obstacle crop")
        counts = np.array([len(s) for s in sets], dtype=np.int64)
        gf = ops.sound_travel_field(free, np.concatenate([[0], np.cumsum(counts)]), np.concatenate(sets), np.array(peaks, np.float32),
                                    decay_rate)
        self._check_bounds(gf, f"sound {sound_name!r}")
        return ops.sound_travel_normalize(gf)

    def index_sound_2d_travel(self, sound_name: str, decay_rate: float = 0.01) -> np.ndarray:
        """index_sound_2d around walls: (h, w) float32 over the obstacle crop.  index_sound_2d's sum -- per segment in order the
        float64 term max(p - (p * d) * decay_rate, 0) added into a float32 field -- with d the TRAVEL distance on the obstacle
        crop from the nearest of the segment's locations (ops.sound_travel_field, csrc/avl_travel_many.hip): a ringing phone is
        colder behind the wall than in front of it, and silent where no walk ends.  Locations outside the crop are dropped, a
        segment with no location left adds nothing; the map is min-max normalised over the crop (index_sound_2d: over the full
        map).  ValueError when no location lies inside the crop or the map is constant."""
        return self._sound_travel_device(sound_name, decay_rate).numpy()

    def index_sound(self, sound_name: str, decay_rate: float = 0.01) -> np.ndarray:
        """(N,) float32.  Reference: avlmap.py:135-144."""
        gf = self._sound_field(sound_name, decay_rate)
        return self._lift(gf, f"sound {sound_name!r}")

    # ------------------------------------------------------------------ image
    def index_image(self, image: np.ndarray, query_cam_intrinsics: np.ndarray = None, decay_rate: float = 0.01) -> np.ndarray:
        """(N,) float64.  Reference: avlmap.py:146-163."""
        from .. import ops
        row, col = self._image_cell(image, query_cam_intrinsics)
        return ops.planar_decay(self.vlmap._device_pos(), row, col, decay_rate).numpy()

    def _image_cell(self, image, query_cam_intrinsics=None):
        """(row, col) of the full map where the query image was taken (avlmap.py:146-153)"""
        if self.visual_map.localizer is None:
            raise MissingSubMap("AVLMap.index_image needs an image localiser (upstream: HLoc): AVLMap(..., localizer=...) or "
                                "visual_map.localizer = ...")
        res = self.visual_map.localize_image(image, query_cam_intrinsic_mat=query_cam_intrinsics)
        if res is None:
            raise ValueError("the query image could not be localised in the map")
        _, query_base_tf = res
        self.dataloader.from_habitat_tf(query_base_tf)
        row, col, _ = self.dataloader.to_full_map_pose()
        return int(row), int(col)

    # ------------------------------------------------------------------ cross-modal goals
    DEFAULT_DECAY = {"obj": 0.1, "area": 0.1, "sound": 0.01, "img": 0.01}     # those of the stand-alone queries

    @staticmethod
    def _goal_specs(obj=None, area=None, sound=None, img=None, extra=(), decay_rates=None):
        """The ordered factor list of a goal: [(modality, what, decay_rate)], objects, areas, sounds, image, extras, each in the
        order given (the float64 product depends on it).  obj / area / sound: a name, a (name, decay_rate) pair, or a list of those."""
        rates = dict(AVLMap.DEFAULT_DECAY)
        for k, v in (decay_rates or {}).items():
            if k not in rates:
                raise ValueError(f"decay_rates: unknown modality {k!r} (one of {sorted(rates)})")
            rates[k] = float(v)

        def is_pair(x):
            return (isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], str)
                    and isinstance(x[1], (int, float, np.integer, np.floating)) and not isinstance(x[1], bool))

        def one(kind, x):
            if isinstance(x, str):
                return (kind, x, rates[kind])
            if is_pair(x):
                return (kind, x[0], float(x[1]))
            raise TypeError(f"{kind}: expected a name or a (name, decay_rate) pair, got {x!r}")

        specs = []
        for kind, arg in (("obj", obj), ("area", area), ("sound", sound)):
            if arg is None:
                continue
            items = [arg] if isinstance(arg, str) or is_pair(arg) else list(arg)
            specs += [one(kind, x) for x in items]
        if img is not None:
            specs.append(("img", img, rates["img"]))
        specs += [("extra", h, None) for h in extra]
        return specs

    def _goal_terms(self, specs, intr_mat=None):
        """ops.GoalTerms of a spec list, built from what the stand-alone queries compute, without their host copies"""
        from .. import ops
        terms = []
        for kind, what, rate in specs:
            if kind == "obj":
                terms.append(ops.GoalTerm.dense(self._object_heat(what, rate)))
            elif kind in ("area", "sound"):
                gf = self._area_field(what, rate) if kind == "area" else self._sound_field(what, rate)
                self._check_bounds(gf, f"{kind} {what!r}")
                terms.append(ops.GoalTerm.field(gf, self._vh()))
            elif kind == "img":
                row, col = self._image_cell(what, intr_mat)
                terms.append(ops.GoalTerm.cones(np.array([[row, col]], dtype=np.int32), np.ones(1), rate))
            else:
                terms.append(ops.GoalTerm.dense(what))
        return terms

    def index_goal(self, obj=None, area=None, sound=None, img=None, intr_mat=None, extra=(), decay_rates=None,
                   want_heat: bool = True) -> "Goal":
        """The cross-modal goal of habitat_lang_robot.py:377-430: the float64 product of the per-voxel heats of every modality
        given, and the first voxel of its maximum, in one pass on the GPU (csrc/avl_goal.hip).

        obj, area, sound: a name, a (name, decay_rate) pair, or a list of those (two objects multiply); img (with intr_mat) as in
        index_image; extra: a sequence of caller-made (N,) heats.  decay_rates={"obj": .., "area": .., "sound": .., "img": ..}
        overrides the stand-alone queries' defaults per modality.  The factors are multiplied in a fixed order: objects, areas,
        sounds, image, extras.  Every factor is the stand-alone query's value bit for bit, so
        goal.heat == float64(index_object(..)) * float64(index_sound(..)) * ... exactly.

        Raises what the stand-alone queries raise; ValueError without any term or on an empty map.  Modalities that do not overlap
        give a product that is 0 everywhere: the goal is then voxel 0 with value 0.0, as np.argmax returns it -- check `value`."""
        specs = self._goal_specs(obj, area, sound, img, extra, decay_rates)
        if not specs:
            raise ValueError("index_goal needs at least one of obj, area, sound, img, extra")
        from .. import ops
        if self.vlmap.grid_pos is None or len(self.vlmap.grid_pos) == 0:
            raise ValueError("an empty map has no goal")
        terms = self._goal_terms(specs, intr_mat)
        res = ops.goal_fuse(terms, self.vlmap._device_pos(), want_heat=want_heat)
        return Goal(res.heat.numpy() if want_heat else None, res.index, res.value, res.pos)

    def index_goal_2d(self, obj=None, area=None, sound=None, decay_rates=None, want_heat: bool = True) -> "Goal2D":
        """The cross-modal goal on the planner's grid: the float64 product of 2-D maps over the obstacle crop
        [rmin:rmax + 1, cmin:cmax + 1] and the cell of its first maximum (habitat_lang_robot.py:357-375 get_map / get_major_map
        and :419-425 get_max_pos), on the GPU (csrc/avl_edt2d.hip, csrc/avl_goal.hip).

        obj, area, sound, decay_rates: as in index_goal, same factor order (objects, areas, sounds).  An object factor is
        vlmap.get_distribution_map(name, rate); an area / sound factor is the crop window of index_area_2d / index_sound_2d as this
        class returns them, i.e. normalised over the FULL map.  The definition is the NumPy product of those stand-alone public
        calls, bit for bit; it makes no claim to equal upstream's region maps, which are built and normalised on the crop.

        Raises what the stand-alone queries raise; ValueError without any term.  goal.cell is a full-map (row, col), what
        Navigator.plan_to takes; goal.value == 0.0 means the modalities do not overlap anywhere on the crop."""
        from .. import ops
        specs = self._goal_specs(obj, area, sound, None, (), decay_rates)
        if not specs:
            raise ValueError("index_goal_2d needs at least one of obj, area, sound")
        if len(specs) > ops.GOAL_MAX_TERMS:
            raise ValueError(f"a goal is the product of 1 to {ops.GOAL_MAX_TERMS} terms, got {len(specs)}")
        vm = self.vlmap
        r0, r1, c0, c1 = vm._crop_window()
        terms = []
        for kind, what, rate in specs:
            if kind == "obj":
                terms.append(vm._distribution_map_device(what, rate))
            else:
                gf = self._area_field(what, rate) if kind == "area" else self._sound_field(what, rate)
                self._check_bounds(gf, f"{kind} {what!r}")
                terms.append(ops.Window(ops.field_normalize(gf), r0, r1, c0, c1))
        res = ops.product_argmax_2d(terms, want_heat=want_heat)
        return Goal2D(res.heat.numpy() if want_heat else None, res.value, (res.cell[0] + r0, res.cell[1] + c0))

    def index_goal_2d_travel(self, obj=None, area=None, sound=None, decay_rates=None, want_heat: bool = True, start=None,
                             start_decay_rate=None) -> "Goal2D":
        """index_goal_2d whose object factors decay around walls: an object factor is vlmap.get_travel_distribution_map(name, rate)
        (csrc/avl_travel.hip), so the goal cell is near the object by the way the robot has to walk, not through the wall behind it.
        Area and sound factors are exactly those of index_goal_2d and stay Euclidean: their fields are maxima over weighted peaks,
        which one distance transform cannot give (index_goal_2d_sound_travel takes the sound factors around walls as well).

        start: the robot's full-map (row, col); it adds one more factor after the others, the UN-normalised travel decay
        ops.travel_decay_2d(get_travel_field([start]), start_decay_rate) from the robot's cell ("the nearest sofa by the way I have
        to walk"); start_decay_rate defaults to 0.01 and is required to be finite and >= 0.  The product and its first maximum go
        through ops.product_argmax_2d like index_goal_2d's: the definition is the NumPy product of the stand-alone public calls, bit
        for bit.  Raises what those calls raise; ValueError without obj, area and sound."""
        return self._goal_2d_travel(obj, area, sound, decay_rates, want_heat, start, start_decay_rate, False)

    def index_goal_2d_sound_travel(self, obj=None, area=None, sound=None, decay_rates=None, want_heat: bool = True, start=None,
                                   start_decay_rate=None) -> "Goal2D":
        """index_goal_2d_travel whose sound factors decay around walls too: every sound factor is index_sound_2d_travel(name, rate)
        -- one travel field per sound segment, in batches (csrc/avl_travel_many.hip), normalised over the crop -- in the place
        index_goal_2d_travel gives the Euclidean one.  Everything else is index_goal_2d_travel's: the arguments, the factor order,
        the object and start factors, the area factor (one cone per frame pose, it stays Euclidean), and the definition as the
        NumPy product of the stand-alone public calls, bit for bit.  Without a sound it is index_goal_2d_travel."""
        return self._goal_2d_travel(obj, area, sound, decay_rates, want_heat, start, start_decay_rate, True)

    def _goal_2d_travel(self, obj, area, sound, decay_rates, want_heat, start, start_decay_rate, sound_travel) -> "Goal2D":
        from .. import ops
        specs = self._goal_specs(obj, area, sound, None, (), decay_rates)
        if not specs:
            raise ValueError("index_goal_2d_travel needs at least one of obj, area, sound")
        if start is None and start_decay_rate is not None:
            raise ValueError("start_decay_rate belongs to start")
        if len(specs) + (start is not None) > ops.GOAL_MAX_TERMS:
            raise ValueError(f"a goal is the product of 1 to {ops.GOAL_MAX_TERMS} terms, got {len(specs) + (start is not None)}")
        vm = self.vlmap
        r0, r1, c0, c1 = vm._crop_window()
        terms = []
        for kind, what, rate in specs:
            if kind == "obj":
                terms.append(vm._travel_distribution_map_device(what, rate))
            elif kind == "sound" and sound_travel:
                terms.append(self._sound_travel_device(what, rate))
            else:
                gf = self._area_field(what, rate) if kind == "area" else self._sound_field(what, rate)
                self._check_bounds(gf, f"{kind} {what!r}")
                terms.append(ops.Window(ops.field_normalize(gf), r0, r1, c0, c1))
        if start is not None:
            field = vm.get_travel_field([start], device=True)
            terms.append(ops.travel_decay_2d(field, 0.01 if start_decay_rate is None else start_decay_rate, device=True))
        res = ops.product_argmax_2d(terms, want_heat=want_heat)
        return Goal2D(res.heat.numpy() if want_heat else None, res.value, (res.cell[0] + r0, res.cell[1] + c0))

    def get_max_pos_3d(self, heat: np.ndarray) -> np.ndarray:
        """grid_pos of the first maximum of a host (N,) float32 / float64 heat.  Reference: habitat_lang_robot.py:427-430."""
        from .. import ops
        heat = np.asarray(heat)
        if heat.dtype not in (np.float32, np.float64):
            raise TypeError(f"heat must be float32 or float64, got {heat.dtype}")
        if heat.shape != (len(self.vlmap.grid_pos),):
            raise ValueError(f"heat must be ({len(self.vlmap.grid_pos)},), got {heat.shape}")
        return ops.goal_fuse([ops.GoalTerm.dense(heat)], self.vlmap._device_pos(), want_heat=False).pos

    # ------------------------------------------------------------------ pictures
    def render_heat(self, heat, view="topdown", transparency: float = 0.5, table=None, size=(640, 480), window=None,
                    intrinsics=None, znear: float = 0.5, smax: float = 16, background=(0, 0, 0)) -> np.ndarray:
        """A uint8 RGB image of a per-voxel heat (what the index_* queries and index_goal(...).heat return; host array or
        DeviceArray, float32 or float64) blended over the map's colours with the colour table (default ops.jet_table()), rendered
        on the GPU from the resident grid_pos and grid_rgb: only the image comes back.

        view="topdown": ops.render_topdown over `window` = (rmin, rmax, cmin, cmax), default the whole (gs, gs) map; `size` is not
        used.  Any other view is a pinhole camera of size = (W, H) through ops.render_view: "frame:<i>" = the camera that took
        frame i (utils.visualize_utils.camera_of_frame: what the robot saw there, coloured by the query), "orbit" = an outside
        view of the whole map (orbit_camera), or a (3, 4) matrix T from cell coordinates to the camera frame (look_at).
        intrinsics = (fx, fy, cx, cy), default the 90-degree pinhole of the simulator's frames for that size."""
        from .. import ops
        from ..utils import visualize_utils as vu
        vm = self.vlmap
        if vm.grid_pos is None or vm.grid_rgb is None:
            raise ValueError("render_heat needs a loaded map with grid_rgb")
        pos, rgb = vm._device_pos(), vm._device_rgb()
        if isinstance(view, str) and view == "topdown":
            return ops.render_topdown(pos, heat, rgb, vm.gs, window=window, transparency=transparency, table=table, background=background)
        if isinstance(view, str) and view == "orbit":
            T = vu.orbit_camera(vm.grid_pos)
        elif isinstance(view, str) and view.startswith("frame:"):
            T = vu.camera_of_frame(vm, int(view[len("frame:"):]))
        elif isinstance(view, str):
            raise ValueError(f"view must be 'topdown', 'orbit', 'frame:<i>' or a (3, 4) matrix, got {view!r}")
        else:
            T = np.asarray(view, dtype=np.float64)
        fx, fy, cx, cy = vu.frame_intrinsics(size) if intrinsics is None else intrinsics
        color = ops.colorize_heat(heat, rgb, transparency, table=table, as_uint8=True, device=True)
        return ops.render_view(pos, color, T, fx, fy, cx, cy, size, znear=znear, smax=smax, background=background)



class Goal:
    """AVLMap.index_goal's answer: heat (N,) float64 (None with want_heat=False), voxel = the first index of its maximum, value =
    the product there (0.0: the modalities do not overlap), pos = grid_pos[voxel] (row, col, height), cell = pos[:2], what
    Navigator.plan_to takes."""
    __slots__ = ("heat", "voxel", "value", "pos")

    def __init__(self, heat, voxel, value, pos):
        self.heat, self.voxel, self.value = heat, int(voxel), float(value)
        self.pos = np.asarray(pos, dtype=np.int32)

    @property
    def cell(self) -> np.ndarray:
        return self.pos[:2]


class Goal2D:
    """AVLMap.index_goal_2d's answer: heat (h, w) float64 over the obstacle crop (None with want_heat=False), value = its maximum
    (0.0: the modalities do not overlap), cell = the full-map (row, col) of the first maximum in raster order, what
    Navigator.plan_to takes."""
    __slots__ = ("heat", "value", "cell")

    def __init__(self, heat, value, cell):
        self.heat, self.value = heat, float(value)
        self.cell = np.asarray(cell, dtype=np.int64)
