"""Camera-pose refinement on the view-matrix gradient of rasterization() / rasterization_3dgs() (gs_project_bwd_view).

``CameraPoseDeltas`` holds one learnable correction per camera and applies it on the right of ``c2w`` (camera-local, so it does not
care that ``Camera.c2w`` is in the OpenGL convention); ``cameras.view_matrix`` of the corrected pose is plain torch, so a loss on the
rendered image reaches the nine numbers of a camera through ``viewmats.grad``.

UNPINNED: this is gsplat's ``CameraOptModule`` as remembered -- translation 3 + a 6-D rotation offset added to the identity's 6-D
code, applied as ``c2w @ delta`` -- not checked against upstream's source.  The semantics written here are the definition.
"""
from __future__ import annotations

from typing import Optional, Union

import torch
from torch import Tensor

from .cameras import Camera


def rot6d(a: Tensor) -> Tensor:
    """[..., 6] -> rotation matrices [..., 3, 3] (Zhou et al., "On the Continuity of Rotation Representations"): b1 = normalize(a1),
    b2 = normalize(a2 - (b1 . a2) b1), b3 = b1 x b2, stacked as ROWS.  (1,0,0,0,1,0) gives the identity exactly."""
    a1, a2 = a[..., :3], a[..., 3:]
    b1 = a1 / a1.norm(dim=-1, keepdim=True)
    b2 = a2 - (b1 * a2).sum(dim=-1, keepdim=True) * b1
    b2 = b2 / b2.norm(dim=-1, keepdim=True)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


class CameraPoseDeltas:
    """One parameter ``deltas`` [num_cameras, 9], zero-initialised: translation (3), then the offset of a 6-D rotation from the
    identity's code (1,0,0,0,1,0).  ``apply(c2w, index)`` = c2w o [rot6d(d[3:] + identity) | d[:3]].

    At zero the slots 3, 6 and 7 have NO gradient, exactly: 3 and 7 move a1 and a2 along themselves, which the two normalisations
    of rot6d remove, and 6 moves a2 along b1, which its Gram-Schmidt step removes.  The other six are the pose's degrees of freedom.
    Not a torch.nn.Module (whose own `apply` means something else): `parameters()` is what an optimizer takes."""

    def __init__(self, num_cameras: int, device=None):
        self.deltas = torch.nn.Parameter(torch.zeros(int(num_cameras), 9, device=device))
        self.identity = torch.zeros(6, device=device)         # filled, not copied from a host list (see cameras.view_matrix)
        self.identity[0].fill_(1.0); self.identity[4].fill_(1.0)

    def parameters(self):
        return [self.deltas]

    def state_dict(self):
        return {"deltas": self.deltas.detach()}

    def load_state_dict(self, state_dict) -> None:
        with torch.no_grad():
            self.deltas.copy_(state_dict["deltas"])

    @property
    def num_cameras(self) -> int:
        return self.deltas.shape[0]

    @torch.no_grad()
    def zero_init_(self) -> "CameraPoseDeltas":
        self.deltas.zero_()
        return self

    @torch.no_grad()
    def random_init_(self, std: float, generator: Optional[torch.Generator] = None) -> "CameraPoseDeltas":
        self.deltas.normal_(0.0, float(std), generator=generator)
        return self

    def apply(self, c2w: Tensor, index: Union[int, Tensor]) -> Tensor:
        """c2w [..., 3, 4] (or [..., 4, 4]) with `index` an int or an int64 tensor [...] on the parameter's device -> the corrected
        pose, same shape.  Zero deltas return c2w's values unchanged."""
        d = self.deltas[index]
        R = rot6d(d[..., 3:] + self.identity)
        Rc, tc = c2w[..., :3, :3], c2w[..., :3, 3:4]
        top = torch.cat((Rc @ R, Rc @ d[..., :3, None] + tc), dim=-1)
        return top if c2w.shape[-2] == 3 else torch.cat((top, c2w[..., 3:, :]), dim=-2)

    def camera(self, cam: Camera, index: Union[int, Tensor]) -> Camera:
        """`cam` with the corrected pose of camera `index` (on the parameter's device)"""
        return Camera(self.apply(cam.c2w.to(self.deltas.device), index), cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
