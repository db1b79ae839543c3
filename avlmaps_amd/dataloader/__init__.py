"""Pose conversion between the Habitat simulator and the map (the reference's avlmaps.dataloader)."""
from .habitat_dataloader import VLMapsDataloaderHabitat  # noqa: F401
