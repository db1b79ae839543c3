"""Host-side mirror of the reference's avlmaps.map builder / indexer interface (VLMap, VLMapBuilder, Map, AVLMap)."""
from .map import Map  # noqa: F401
from .vlmap import VLMap  # noqa: F401
from .vlmap_builder import VLMapBuilder  # noqa: F401
from .avlmap import AVLMap, Goal, Goal2D  # noqa: F401
from .vlmap_builder_multi_floor import VLMapBuilderMultiFloor  # noqa: F401
from .vlmap_multi_floor import VLMapMultiFloor  # noqa: F401
from .gtmap import GTMap  # noqa: F401
from .rooms import Rooms  # noqa: F401
from .tour import Tour, TOUR_MAX_GOALS  # noqa: F401
