// host_capi.cpp -- C entry points of the host mirror used by the Python side.
#include "acoustic_model.hpp"
#include "elastic_model.hpp"

extern "C" {

/// ElasticModel<D>::constructGcmMatrices for an isotropic material, identity
/// basis: U, U1 [D][M*M] row-major, L [D][M].  Returns 0 or -1 (bad input).
int gcm_host_isotropic_elastic_matrices(int D, double rho, double lambda, double mu, double* U,
                                        double* U1, double* L) {
	try {
		auto run = [&](auto tag) {
			constexpr int DD = decltype(tag)::value;
			constexpr int M = gcm::pdeSize(DD);
			gcm::GcmMatrices<DD> m;
			gcm::ElasticModel<DD>::constructGcmMatrices(m, gcm::IsotropicMaterial(rho, lambda, mu));
			for (int s = 0; s < DD; s++) {
				for (int i = 0; i < M * M; i++) {
					U[s * M * M + i] = m.m[s].U[i];
					U1[s * M * M + i] = m.m[s].U1[i];
				}
				for (int k = 0; k < M; k++) L[s * M + k] = m.m[s].L[k];
			}
		};
		switch (D) {
		case 1: run(std::integral_constant<int, 1>()); return 0;
		case 2: run(std::integral_constant<int, 2>()); return 0;
		case 3: run(std::integral_constant<int, 3>()); return 0;
		default: return -1;
		}
	} catch (...) {
		return -1;
	}
}

/// ElasticModel<3>::constructGcmMatrices for an unrotated orthotropic material
/// (c = c11, c12, c13, c22, c23, c33, c44, c55, c66): U, U1 [3][81] row-major,
/// L [3][9].  Returns 0 or -1 (bad input).
int gcm_host_orthotropic_elastic_matrices(double rho, const double* c, double* U, double* U1, double* L) {
	try {
		gcm::GcmMatrices<3> m;
		gcm::ElasticModel<3>::constructGcmMatrices(
		    m, gcm::OrthotropicMaterial(rho, {c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]}));
		for (int s = 0; s < 3; s++) {
			for (int i = 0; i < 81; i++) {
				U[s * 81 + i] = m.m[s].U[i];
				U1[s * 81 + i] = m.m[s].U1[i];
			}
			for (int k = 0; k < 9; k++) L[s * 9 + k] = m.m[s].L[k];
		}
		return 0;
	} catch (...) {
		return -1;
	}
}

/// AcousticModel<D>::constructGcmMatrices for an isotropic material (mu unused),
/// identity basis: U, U1 [D][M*M] row-major, L [D][M], M = D + 1.  Returns 0 or
/// -1 (bad input).
int gcm_host_acoustic_matrices(int D, double rho, double lambda, double mu, double* U, double* U1, double* L) {
	try {
		auto run = [&](auto tag) {
			constexpr int DD = decltype(tag)::value;
			constexpr int M = gcm::acousticPdeSize(DD);
			gcm::AcousticMatrices<DD> m;
			gcm::AcousticModel<DD>::constructGcmMatrices(m, gcm::IsotropicMaterial(rho, lambda, mu));
			for (int s = 0; s < DD; s++) {
				for (int i = 0; i < M * M; i++) {
					U[s * M * M + i] = m.m[s].U[i];
					U1[s * M * M + i] = m.m[s].U1[i];
				}
				for (int k = 0; k < M; k++) L[s * M + k] = m.m[s].L[k];
			}
		};
		switch (D) {
		case 1: run(std::integral_constant<int, 1>()); return 0;
		case 2: run(std::integral_constant<int, 2>()); return 0;
		case 3: run(std::integral_constant<int, 3>()); return 0;
		default: return -1;
		}
	} catch (...) {
		return -1;
	}
}

/// OrthotropicMaterial(const IsotropicMaterial&): the nine constants, in constructor order.
void gcm_host_orthotropic_from_isotropic(double rho, double lambda, double mu, double* c) {
	const gcm::OrthotropicMaterial m(gcm::IsotropicMaterial(rho, lambda, mu));
	for (int i = 0; i < 9; i++) c[i] = m.c[i];
}

}
