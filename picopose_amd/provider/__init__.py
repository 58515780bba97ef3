"""Mirror of the reference's provider/: training-pair assembly on the device (training_batch), a test image's detection
batch from its RLE records (test_batch) and an object's template bank from its mesh (template_bank)."""
from .template_bank import (TEMPLATE_K, Shading, load_model, load_ply, load_texture, mesh_diameter, onboard_objects,  # noqa: F401
                            render_templates, render_views, srgb_tone_table, template_lights, template_object_poses,
                            templates_from_frames, vertex_normals)
