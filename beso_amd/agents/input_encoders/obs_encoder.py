"""Boundary plumbing of the agent: which entries of a batch dict are the observation window and the goal,
and on which device the score network wants them (interface of the reference's
beso/agents/input_encoders/obs_encoder.py:11-21: constructor kwargs ``device, state_modality,
goal_modality``; ``forward(batch) -> (state, goal-or-None)``)."""
from typing import Optional, Tuple

import torch
from torch import Tensor, nn


class NoEncoder(nn.Module):
    """Identity "encoder": observations are already feature vectors (kitchen / block-push)."""

    def __init__(self, device: str, state_modality: str, goal_modality: str):
        super().__init__()
        self.device = device
        self.state_modality, self.goal_modality = state_modality, goal_modality

    def _fetch(self, batch: dict, key: str) -> Optional[Tensor]:
        value = batch.get(key)
        return None if value is None else value.to(self.device, non_blocking=True)

    @torch.no_grad()
    def forward(self, batch: dict) -> Tuple[Tensor, Optional[Tensor]]:
        state = self._fetch(batch, self.state_modality)
        if state is None:
            raise KeyError(self.state_modality)
        return state, self._fetch(batch, self.goal_modality)


class MLPEncoder(NoEncoder):
    """A trainable ``MLPNetwork`` (beso_amd/networks/mlps/mlps.py: HIP kernels, forward and backward) in front of the score
    network, for observations that are not the denoiser's ``obs_dim`` features.  The reference ships no trainable encoder;
    its ``MLPNetwork`` (networks/mlps/mlps.py:11-73) is the only small network it has for the role.

    ``network`` is a config for ``MLPNetwork`` (``_target_`` + kwargs) or a factory.  ``forward(batch)`` fetches exactly as
    ``NoEncoder.forward`` does -- ``BaseAgent.process_batch`` and the scaler see the RAW observations; the agent scales
    first and encodes second -- and ``encode(state, goal)`` maps the last dimension of both through the ONE shared network,
    keeping the leading dimensions.  With ``encode_goal=False`` the goal passes through."""

    def __init__(self, device: str, state_modality: str, goal_modality: str, network, encode_goal: bool = True):
        super().__init__(device, state_modality, goal_modality)
        from ..._instantiate import instantiate
        self.network = instantiate(network)
        self.network.get_device(device)
        self.encode_goal = bool(encode_goal)

    def get_params(self):
        return self.network.get_params()

    def encode(self, state: Tensor, goal: Optional[Tensor]) -> Tuple[Tensor, Optional[Tensor]]:
        state_e = self.network(state)
        if goal is None or not self.encode_goal:
            return state_e, goal
        return state_e, self.network(goal)
