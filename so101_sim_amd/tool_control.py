"""Cartesian tool control shared by the batched environments (`BatchedEnvironment` of env.py on the SO100 engine, `AlohaEnvironment`
of aloha.py on the general-tree engine): argument handling and output allocation of `tool_pose` and `solve_ik`.

An environment supplies `_resolve_tool(tool)` (a tools.Tool with the body numbering of its engine), `_tool_columns(t)` (the columns of q and
of the Jacobian for that tool) and `_ik_config(t, mode, config)` (the settings struct of its native handle), and keeps its own public
`tool_pose` / `solve_ik` with its default tool and documentation; `self.sim` has tool_pose / tool_ik (native.Sim, native.TreeSim).
"""
from __future__ import annotations

import numpy as np


class ToolControl:
    def _env_index(self, env_ids):
        """env_ids (sequence, tensor or None) -> (int32 device tensor or None, count)"""
        if env_ids is None:
            return None, self.n_envs
        torch = self.torch
        idx = torch.as_tensor(env_ids, dtype=torch.int32, device=self.device).reshape(-1).contiguous()
        n = int(idx.numel())
        if n == 0 or int(idx.min()) < 0 or int(idx.max()) >= self.n_envs:
            raise ValueError("env_ids must name at least one env of this batch")
        return idx, n

    def _f32(self, a):
        """array-like or tensor -> float32 tensor on the env's device (numpy input is copied: it may be read-only)"""
        if isinstance(a, np.ndarray):
            a = np.array(a, dtype=np.float32)
        return self.torch.as_tensor(a, dtype=self.torch.float32, device=self.device)

    def _joint_rows(self, q, ncol, what):
        q = self._f32(q)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if q.dim() != 2 or q.shape[1] != ncol or q.shape[0] < 1:
            raise ValueError(f"{what} must be [n, {ncol}] joint values of the tool's chain, got {tuple(q.shape)}")
        return q.contiguous()

    def _tool_pose(self, tool, env_ids, q, jacobian):
        torch = self.torch
        t = self._resolve_tool(tool)
        ncol = self._tool_columns(t)
        if q is not None:
            if env_ids is not None:
                raise ValueError("env_ids selects envs of the current state: it cannot be combined with q")
            q = self._joint_rows(q, ncol, "q")
            idx, n = None, int(q.shape[0])
        else:
            idx, n = self._env_index(env_ids)
        pos = torch.empty(n, 3, dtype=torch.float32, device=self.device)
        mat = torch.empty(n, 3, 3, dtype=torch.float32, device=self.device)
        jac = torch.empty(n, 6, ncol, dtype=torch.float32, device=self.device) if jacobian else None
        self.sim.tool_pose(t.spec(), q.data_ptr() if q is not None else None, idx.data_ptr() if idx is not None else None, n,
                           pos.data_ptr(), mat.data_ptr(), jac.data_ptr() if jac is not None else None, self._stream())
        return (pos, mat, jac) if jacobian else (pos, mat)

    def _solve_ik(self, target_pos, target_mat, tool, mode, q_init, env_ids, config):
        torch = self.torch
        t = self._resolve_tool(tool)
        ncol = self._tool_columns(t)
        tp = self._f32(target_pos)
        if tp.dim() == 1:
            tp = tp.unsqueeze(0)
        if tp.dim() != 2 or tp.shape[1] != 3 or tp.shape[0] < 1:
            raise ValueError(f"target_pos must be [n, 3], got {tuple(tp.shape)}")
        tp = tp.contiguous()
        n = int(tp.shape[0])
        tm = None
        if target_mat is not None:
            tm = self._f32(target_mat).reshape(-1, 3, 3).contiguous()
            if tm.shape[0] != n:
                raise ValueError(f"target_mat must be [{n}, 3, 3], got {tuple(tm.shape)}")
        if mode is None:
            mode = 0 if tm is None else 1
        if q_init is not None:
            if env_ids is not None:
                raise ValueError("env_ids selects envs of the current state: it cannot be combined with q_init")
            q_init = self._joint_rows(q_init, ncol, "q_init")
            if q_init.shape[0] != n:
                raise ValueError(f"q_init must be [{n}, {ncol}], got {tuple(q_init.shape)}")
            idx = None
        else:
            idx, k = self._env_index(env_ids)
            if idx is not None and k != n:
                raise ValueError(f"env_ids names {k} envs for {n} targets")
        cfg = self._ik_config(t, int(mode), config)
        q = torch.empty(n, ncol, dtype=torch.float32, device=self.device)
        residual = torch.empty(n, 2, dtype=torch.float32, device=self.device)
        iters = torch.empty(n, dtype=torch.int32, device=self.device)
        self.sim.tool_ik(t.spec(), cfg, tp.data_ptr(), tm.data_ptr() if tm is not None else None,
                         q_init.data_ptr() if q_init is not None else None, idx.data_ptr() if idx is not None else None, n,
                         q.data_ptr(), residual.data_ptr(), iters.data_ptr(), self._stream())
        return q, iters >= 0, residual, iters
