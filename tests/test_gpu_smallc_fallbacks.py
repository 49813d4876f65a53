"""The output layer's fallbacks that a shape alone reaches (output layer: reachability table).

Channel counts no golden case has: the register-resident and generic kernels of csrc/smallc.hip run only
where the two-stage forward (Cin % 8 == 0, Cout 1 or 3) and the k3 dgrad kernel do not apply.  Each case is
a tiny drop-in generator through the normal Python path, checked against the oracle with the criterion of
test_gpu_langevin.py::test_cifar_b128_step_vs_oracle: the HIP result's distance to an fp64 evaluation stays
within 3x the fp32 reference arithmetic's own (+ 1e-6), and within the file's gradient bound (1e-5) of the
fp32 oracle.  (The oracle's fp32-against-fp64 distance for these gradients is 3.0e-7 .. 6.2e-7.)

The kernels each case reaches (smallc_fwd_path / smallc_dgrad_kernel_of in csrc/smallc.hip; none of these
nets has a limb-engine layer, so no sign bits and no limbs are involved):

  case            output layer      forward                         dgrad
  cifar10_ngf2    k3 s1, 4 -> 3     smallc_fwd_reg_kernel<3,3,1,4>  smallc_dgrad_reg_kernel<3,3,1,4>
  mnist_ngf2      k3 s1, 4 -> 1     smallc_fwd_reg_kernel<1,3,1,4>  smallc_dgrad_reg_kernel<1,3,1,4>
  svhn_ngf1       k4 s2, 2 -> 3     smallc_fwd_s2_kernel<3,2>       smallc_dgrad_reg_kernel<3,4,2,2>
  cifar10_ngf1    k3 s1, 2 -> 3     smallc_fwd_kernel<3>            smallc_dgrad_kernel<3>
  svhn_ngf3       k4 s2, 6 -> 3     smallc_fwd_kernel<3>            smallc_dgrad_kernel<3>   (stride 2)
  cifar10_nc4     k3 s1, 8 -> 4     smallc_fwd_kernel<4>            smallc_dgrad_kernel<4>
  cifar10_nc2     k3 s1, 8 -> 2     smallc_fwd_kernel<2>            smallc_dgrad_kernel<2>
"""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

B, NZ, SIGMA = 3, 16, 0.1

# name: (constructor, ngf, nc, image side)
CASES = {
    "cifar10_ngf2": ("_netG_cifar10", 2, 3, 32),
    "mnist_ngf2": ("_netG_mnist", 2, 1, 28),
    "svhn_ngf1": ("_netG_svhn", 1, 3, 32),
    "cifar10_ngf1": ("_netG_cifar10", 1, 3, 32),
    "svhn_ngf3": ("_netG_svhn", 3, 3, 32),
    "cifar10_nc4": ("_netG_cifar10", 4, 4, 32),
    "cifar10_nc2": ("_netG_cifar10", 4, 2, 32),
}


@pytest.mark.parametrize("name", list(CASES))
def test_output_layer_fallback_vs_oracle(gpu_device, name):
    from damc import langevin as lv
    from damc import synth
    from oracle import damc_oracle as orc
    from src import diffusion_net as dn

    ctor, ngf, nc, H = CASES[name]
    G = synth.load_into(getattr(dn, ctor)(nz=NZ, ngf=ngf, nc=nc), 0).to(gpu_device).eval()
    x = torch.from_numpy(synth.uniform_f32(1, 0, (B, nc, H, H)))
    z = torch.from_numpy(synth.normal_f32(2, 0, (B, NZ)))
    L32, L64 = orc.generator_layers(G), orc.generator_layers(G, torch.float64)

    xh = lv.generator_forward(z.to(gpu_device), G).cpu().numpy()
    xh32 = orc.generator_sample(L32, z).numpy()
    xh64 = orc.generator_sample(L64, z.double()).numpy()
    print("%s forward: hip-fp64 %.3e oracle32-fp64 %.3e hip-oracle32 %.3e"
          % (name, rel_l2(xh, xh64), rel_l2(xh32, xh64), rel_l2(xh, xh32)))
    g = lv.likelihood_grad(z.to(gpu_device), x.to(gpu_device), G, SIGMA).cpu().numpy()
    g32 = orc.likelihood_grad(L32, z, x, SIGMA)[0].numpy()
    g64 = orc.likelihood_grad(L64, z.double(), x.double(), SIGMA)[0].numpy()
    print("%s gradient: hip-fp64 %.3e oracle32-fp64 %.3e hip-oracle32 %.3e"
          % (name, rel_l2(g, g64), rel_l2(g32, g64), rel_l2(g, g32)))

    assert xh.shape == xh32.shape
    assert rel_l2(xh, xh64) <= 3 * rel_l2(xh32, xh64) + 1e-6
    assert rel_l2(xh, xh32) < 1e-5
    assert rel_l2(g, g64) <= 3 * rel_l2(g32, g64) + 1e-6
    assert rel_l2(g, g32) < 1e-5
