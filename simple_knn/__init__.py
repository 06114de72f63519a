"""Drop-in for upstream 3DGS's `simple_knn` extension: `from simple_knn._C import distCUDA2` resolves to the exact k-NN
kernel of gaussreg_amd.scene_init."""
