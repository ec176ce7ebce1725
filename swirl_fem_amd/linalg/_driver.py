"""What the Krylov solvers share around their iteration: the graph capture, the
driver loop, the kept solver states and the breakdown warning."""

from __future__ import annotations

import gc
import warnings

import torch


def capture_graph(record):
  """Records the device work of `record()` into a HIP graph; returns the
  graph, or None if something in it cannot be captured (the device is then
  synchronised; whatever the caller counted or kept is the caller's to undo).

  The cyclic collector must not run while the stream is capturing: an older
  solver state that sits in a reference cycle (stepper -> cache -> runner ->
  operator -> stepper) owns a graph and its memory pool, and freeing those in
  the middle of a capture aborts the process.  Collect first, then keep the
  collector off until the capture has ended.
  """
  graph = torch.cuda.CUDAGraph()
  gc.collect()
  was_enabled = gc.isenabled()
  gc.disable()
  try:
    with torch.cuda.graph(graph):
      record()
  except Exception:                # pylint: disable=broad-except
    torch.cuda.synchronize()
    return None
  finally:
    if was_enabled:
      gc.enable()
  return graph


def drive(run, check_every):
  """Steps `run` until its device flag reports the end or `maxiter` is
  reached; the host polls the flag every `check_every` iterations."""
  while run.issued < run.maxiter:
    for _ in range(min(check_every, run.maxiter - run.issued)):
      run.step()
    if run.done():
      break


def kept_runner(workspace, key, limit, fits, make):
  """`(run, kept)`: the solver state under `workspace[key]` if `fits(run)`
  (the caller restarts it), else `make()`, kept there in its place -- or kept
  nowhere without a workspace.  The most recently used state goes last and
  the oldest ones beyond `limit` go: a stepper whose coefficients change every
  step must not collect solver states without bound."""
  if workspace is None:
    return make(), False
  run = workspace.get(key)
  if run is not None and fits(run):
    workspace[key] = workspace.pop(key)
    return run, True
  run = make()
  workspace.pop(key, None)
  workspace[key] = run
  while len(workspace) > limit:
    workspace.pop(next(iter(workspace)))
  return run, False


def warn_on_breakdown(solver, info):
  """A RuntimeWarning, attributed to the caller of the solver, when the solve
  ended in a breakdown: the reference would have returned that as a converged
  solve; callers that ignore `info` (the Stokes solves) at least get told."""
  status = info['status']
  if not status.startswith('breakdown'):
    return
  if 'member_status' in info:
    text = (f"{solver}: a member stopped with status '{status}': its x is "
            'the last iterate, not a solution to the requested tolerance')
  else:
    text = (f"{solver} stopped with status '{status}' after "
            f"{info['num_iterations']} iterations: x is the last iterate, "
            'not a solution to the requested tolerance')
  # (1: here, 2: cg / cg_ensemble / bicgstab, 3: who called them)
  warnings.warn(text, RuntimeWarning, stacklevel=3)
