from .render import Mesh, MeshRenderer, load_obj  # noqa: F401
from .scene import SceneRenderer, make_scene_frames, sample_scenes  # noqa: F401
