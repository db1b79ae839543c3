"""Sound-category helpers with the reference's names (avlmaps/utils/audio_utils.py)."""
from __future__ import annotations

from typing import List


def get_level_categories(difficulty_level: str, sound_config) -> List[str]:
    """Sorted sound categories of a difficulty level: the union of its major categories' classes, '_' read as ' '.
    Reference: audio_utils.py:230-236."""
    major2categories = sound_config["major_categories"]
    cats = []
    for major in sound_config["difficulty"][difficulty_level]:
        cats.extend([x.replace("_", " ") for x in major2categories[major]])
    return sorted(cats)
