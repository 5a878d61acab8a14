"""Drop-in for scipy.cluster.vq in the demos (kmeans(Xtrain, num_ind, seed=0)[0])."""
from modulatedgps_amd.cluster import kmeans, kmeans_device, vq, vq_device  # noqa: F401
