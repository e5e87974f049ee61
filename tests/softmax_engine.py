"""TEST DOUBLE (as tests/cpu_engine.py, which it extends): ``NumpyShardEngine`` plus the coupled Softmax map, so that the host
logic around the Softmax likelihood -- constructor and target checks, the draw bookkeeping, row offsets over ranks, the site
update -- runs on CPU.  The map here is the NumPy restatement (tests/softmax_ref.py) at the product likelihood's
(seed, draw, row_offset); like ``EStepEngine.lik_map`` it advances the likelihood's draw once per evaluation."""
import numpy as np
import torch

from oracle import tsvgp_oracle as O
from tests.cpu_engine import NumpyShardEngine, _Stats
from tests.softmax_ref import Softmax as RefSoftmax

LIK_SOFTMAX = 4
_TRI = {0: np.tril, 1: np.triu, 2: lambda a: a}


def _pick(T, p):
    if T is None:
        return None
    if isinstance(T, (list, tuple)):
        return T[p]
    return T[p] if T.dim() == 3 else T


class CoupledNumpyEngine(NumpyShardEngine):
    def run(self, X, Y, Z, kernel, *, moment_Tm, moment_mode, gamma, lik_id=0, lik_param=0.0, whiten_T=None, whiten_mode=1,
            project_T=None, sites=False, want_moments=False, want_grads=False, project_mode=0, moments_on_kfu=False, **kw):
        if (lik_id & 0xFF) != LIK_SOFTMAX:
            return super().run(X, Y, Z, kernel, moment_Tm=moment_Tm, moment_mode=moment_mode, gamma=gamma, lik_id=lik_id,
                               lik_param=lik_param, whiten_T=whiten_T, whiten_mode=whiten_mode, project_T=project_T, sites=sites,
                               want_moments=want_moments, want_grads=want_grads, project_mode=project_mode,
                               moments_on_kfu=moments_on_kfu, **kw)
        lik = lik_param
        P = moment_Tm.shape[0]
        if P != lik.latent_dim or Y is None or Y.dim() != 2 or Y.shape[1] != 1 or Y.shape[0] != X.shape[0]:
            raise ValueError("the Softmax likelihood needs latent_dim latent GPs and Y [N, 1]")
        base = super().run(X, None, Z, kernel, moment_Tm=moment_Tm, moment_mode=moment_mode, gamma=gamma, whiten_T=whiten_T,
                           whiten_mode=whiten_mode, want_moments=True, moments_on_kfu=moments_on_kfu)
        mean, var = base.mean.numpy(), base.var.numpy()
        ref = RefSoftmax(lik.num_classes, lik.seed)
        ref.num_monte_carlo_points = lik.num_monte_carlo_points
        ref.draw, ref.row_offset = lik.draw, lik.row_offset
        Yn = Y.cpu().numpy()
        eps = ref._eps(len(Yn), None)
        g0, g1 = ref.variational_expectations_grads(mean, var, Yn, epsilon=eps)
        if not (lik_id & 0x100):
            g1 = np.minimum(g1, -1e-8)
        lik.advance()
        st = _Stats()
        st.n_rows, st.nonpos = base.n_rows, base.nonpos
        st.ve_sum = torch.tensor(float(np.sum(ref.variational_expectations(mean, var, Yn, epsilon=eps))), dtype=torch.float64)
        st.mean, st.var = (base.mean, base.var) if want_moments else (None, None)
        st.g0, st.g1 = (torch.as_tensor(g0), torch.as_tensor(g1)) if want_grads else (None, None)
        st.acc2 = st.acc1 = None
        if sites:
            Xn, Zn = X.cpu().numpy(), Z.cpu().numpy()
            kernels = kernel.kernels if hasattr(kernel, "kernels") else [kernel] * P
            acc2, acc1 = [], []
            for p, kp in enumerate(kernels):
                k = getattr(O, type(kp).__name__)(variance=float(kp.variance.value), lengthscales=kp.lengthscales.numpy())
                A = k.K(Xn, Zn)
                shared = not hasattr(kernel, "kernels")
                wT = whiten_T if shared else _pick(whiten_T, p)
                pT = project_T if shared else _pick(project_T, p)
                if wT is not None:
                    A = A @ _TRI[whiten_mode](wT.cpu().numpy()).T
                if pT is not None:
                    A = A @ _TRI[project_mode](pT.cpu().numpy()).T
                acc2.append(np.einsum("nm,no,n->mo", A, A, g1[:, p]))
                acc1.append(A.T @ g0[:, p])
            st.acc2, st.acc1 = torch.as_tensor(np.stack(acc2)), torch.as_tensor(np.stack(acc1))
        return st
