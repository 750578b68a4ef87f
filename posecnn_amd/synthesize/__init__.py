from .render import Mesh, MeshRenderer, load_obj  # noqa: F401
from .scene import SceneRenderer, make_scene_frames, sample_scenes  # noqa: F401
from .image import (PIXEL_MEANS, LitSceneRenderer, image_blob, make_image_frames, sample_jitter,  # noqa: F401
                    sample_lights)
