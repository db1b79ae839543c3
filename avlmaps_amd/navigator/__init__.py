from .navigator import Navigator, NoPathError  # noqa: F401
