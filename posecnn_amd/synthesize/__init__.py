from .render import Mesh, MeshRenderer, load_obj  # noqa: F401
