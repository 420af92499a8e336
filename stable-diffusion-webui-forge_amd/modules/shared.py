"""The few globals of modules/shared.py the path reads (state flags, opts), without gradio.
Defaults follow modules/shared_options.py (randn_source :185, s_min_uncond :239, skip_early_cond :416,
eta_noise_seed_delta :408, always_discard_next_to_last_sigma :409, sgm_noise_multiplier :410,
use_old_karras_scheduler_sigmas :256, beta_dist_alpha/beta :417-418, uni_pc_* :411-414, sd_vae_encode_method / sd_vae_decode_method :213-214,
live_previews_enable :383, show_progress_every_n_steps :386, show_progress_type :387) and modules/shared_state.py.

Live previews: `live_previews_enable` is False here where the reference's default is True -- with it off the sampler launches exactly what it
launched before previews existed (the bench, the tests and every existing caller), and a library has no UI to show them in; a caller that wants
them sets it (and `show_progress_type`, "TAESD" for the native tiny decoder).  `show_progress_grid` is not mirrored: previews show sample 0."""
from types import SimpleNamespace

opts = SimpleNamespace(
    randn_source="CPU",  # reference default is "GPU"; "CPU"/"NV" are the device-independent sources (modules/rng.py:6-33)
    eta_noise_seed_delta=0, always_discard_next_to_last_sigma=False, sgm_noise_multiplier=False,
    use_old_karras_scheduler_sigmas=False, s_min_uncond=0.0, s_min_uncond_all=False, skip_early_cond=0.0,
    eta_ancestral=1.0, eta_ddim=0.0, sigma_min=0.0, sigma_max=0.0, rho=0.0, s_churn=0.0, s_tmin=0.0, s_tmax=0.0, s_noise=1.0,
    uni_pc_variant="bh1", uni_pc_skip_type="time_uniform", uni_pc_order=3, uni_pc_lower_order_final=True, beta_dist_alpha=0.6, beta_dist_beta=0.6, forge_try_reproduce="None", sd_vae_decode_method="Full",
    sd_vae_encode_method="Full", live_previews_enable=False, show_progress_every_n_steps=10, show_progress_type="Approx NN",
    ESRGAN_tile=192, ESRGAN_tile_overlap=8, upscaler_for_img2img=None,  # modules/shared_options.py:102-103,108
)


class State:
    def __init__(self):
        self.interrupted = False
        self.skipped = False
        self.sampling_step = 0
        self.sampling_steps = 0
        self.current_latent = None
        self.current_image = None                 # shared_state.py:28-30
        self.current_image_sampling_step = 0
        self.id_live_preview = 0

    def interrupt(self):
        self.interrupted = True

    def set_current_image(self):
        """shared_state.py:145-152: for a caller that polls from another thread (`parallel_processing_allowed`): if enough sampling steps have
        been made after the last preview, sets current_image from current_latent and moves id_live_preview"""
        if not parallel_processing_allowed:
            return
        if self.sampling_step - self.current_image_sampling_step >= opts.show_progress_every_n_steps and opts.live_previews_enable and opts.show_progress_every_n_steps != -1:
            self.do_set_current_image()

    def do_set_current_image(self):
        """shared_state.py:154-175 without the grid (sample 0) and without swallowing errors"""
        if self.current_latent is None:
            return
        from . import sd_samplers_common
        self.assign_current_image(sd_samplers_common.sample_to_image(self.current_latent))
        self.current_image_sampling_step = self.sampling_step

    def assign_current_image(self, image):
        """shared_state.py:184-190"""
        self.current_image = image
        self.id_live_preview += 1


state = State()
sd_model = None
sd_upscalers = []                    # UpscalerData entries by name (modules/shared.py sd_upscalers); modules/esrgan_model.register() fills it
device = None
models_path = "models"               # modules/paths_internal.py models_path: TAESD weights are looked up in <models_path>/VAE-taesd (modules/sd_vae_taesd.py)
parallel_processing_allowed = False  # shared.py:60-ish of the reference: True there when a UI thread polls State.set_current_image; here the sampler makes the previews itself
