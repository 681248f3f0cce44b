"""The reference's generation-side library (SG3/genlib): the latent projector."""
