// acoustic_model.hpp -- host-side GcmMatrices for acoustic media.
//
// Mirrors rheology/models/AcousticModel.hpp:214-317 (constructGcmMatrices,
// constructGcmMatrix, constructEigenvectors, constructEigenstrings) for the
// identity calculation basis the cubic engine uses, and the quantity map of
// rheology/variables/AcousticVariables.hpp.  The PDE vector is the velocity
// (D components), then the pressure at index D: M = D + 1.  Every expression
// keeps the reference's evaluation order so the tables are bitwise the
// reference's (checked against a numpy restatement in tests/test_acoustic_cpu.py).
#pragma once

#include <cmath>
#include <string>

#include "task.hpp"

namespace gcm {

constexpr int acousticPdeSize(int D) { return D + 1; }

/// GcmMatrices<D + 1, D> (util/math/GridCharacteristicMethod.hpp:40-110), row-major.
template <int D>
struct AcousticMatrices {
	static constexpr int M = acousticPdeSize(D);
	struct GcmMatrix {
		std::array<real, M * M> A{}, U{}, U1{};
		std::array<real, M> L{};
		real getMaximalEigenvalue() const {
			real ans = 0;
			for (int i = 0; i < M; i++) ans = std::fmax(ans, std::fabs(L[i]));
			return ans;
		}
		/// GcmMatrix::checkDecomposition (GridCharacteristicMethod.hpp:60-69)
		void checkDecomposition(const real eps) const {
			auto at = [](const std::array<real, M * M>& a, int i, int j) { return a[i * M + j]; };
			real trA = 0, trL = 0;
			for (int i = 0; i < M; i++) {
				trA += at(A, i, i);
				trL += L[i];
			}
			bool ok = std::fabs(trA - trL) <= eps;
			for (int i = 0; i < M && ok; i++)
				for (int j = 0; j < M && ok; j++) {
					real au1 = 0, ua = 0, uu1 = 0;
					for (int k = 0; k < M; k++) {
						au1 += at(A, i, k) * at(U1, k, j);
						ua += at(U, i, k) * at(A, k, j);
						uu1 += at(U, i, k) * at(U1, k, j);
					}
					ok = std::fabs(au1 - at(U1, i, j) * L[j]) <= eps * 1000 &&
					     std::fabs(ua - L[i] * at(U, i, j)) <= eps * 1000 &&
					     std::fabs(uu1 - (i == j ? 1.0 : 0.0)) <= eps * 1000;
				}
			if (!ok) throw Exception("AcousticModel: the GCM matrices do not decompose A");
		}
	};
	GcmMatrix m[D];
	real getMaximalEigenvalue() const {
		real ans = 0;
		for (int i = 0; i < D; i++) ans = std::fmax(ans, m[i].getMaximalEigenvalue());
		return ans;
	}
};

/// AcousticModel<D> (rheology/models/AcousticModel.hpp) -- matrix construction only.
template <int D>
struct AcousticModel {
	static constexpr int DIMENSIONALITY = D;
	static constexpr int PDE_SIZE = acousticPdeSize(D);
	static constexpr real EQUALITY_TOLERANCE = 1e-9;  // util/infrastructure/Types.hpp:10
	using Matrices = AcousticMatrices<D>;

	/// constructGcmMatrices with the identity basis.  Only rho and lambda enter;
	/// mu is unused and may be 0 (the launcher's acoustic task passes
	/// IsotropicMaterial(1, 1, 0), launcher/main.cpp:422-467).
	static void constructGcmMatrices(Matrices& out, const IsotropicMaterial& mat) {
		if (!(mat.rho > 0) || !(mat.lambda > 0)) throw Exception("acoustic material needs rho > 0 and lambda > 0");
		for (int i = 0; i < D; i++) {
			real basis[D][D] = {};
			detail::localBasis<D>(i, basis);
			constructGcmMatrix(out.m[i], mat, basis);
		}
	}

	/// AcousticModel.hpp:214-245 with l = 1
	static void constructGcmMatrix(typename Matrices::GcmMatrix& m, const IsotropicMaterial& mat,
	                               const real basis[D][D], const real l = 1) {
		constexpr int M = PDE_SIZE;
		const real rho = mat.rho;
		const real lambda = mat.lambda;
		const real c1 = std::sqrt(lambda / rho);
		m.A.fill(0);
		m.U.fill(0);
		m.U1.fill(0);
		m.L.fill(0);
		// n[0] = the normal (the basis's last column), then the tangents, signs included
		real n[D][D];
		for (int i = 0; i < D; i++)
			for (int r = 0; r < D; r++) n[i][r] = basis[r][(i + D - 1) % D];

		// A along n with scale l: row D = {l lambda n, 0}, column D = {l / rho n, 0}
		for (int r = 0; r < D; r++) m.A[D * M + r] = n[0][r] * (l * lambda);
		m.A[D * M + D] = 0;
		for (int r = 0; r < D; r++) m.A[r * M + D] = n[0][r] * (l / rho);
		m.A[D * M + D] = 0;

		m.L[0] = l * c1;
		m.L[1] = -l * c1;

		// constructEigenvectors (:248-280): columns of U1
		{
			real pressure = c1 * rho;
			for (int r = 0; r < D; r++) m.U1[r * M + 0] = n[0][r];
			m.U1[D * M + 0] = pressure;
			pressure = -pressure;
			for (int r = 0; r < D; r++) m.U1[r * M + 1] = n[0][r];
			m.U1[D * M + 1] = pressure;
			for (int i = 1; i < D; i++) {
				for (int r = 0; r < D; r++) m.U1[r * M + (i + 1)] = n[i][r];
				m.U1[D * M + (i + 1)] = 0;
			}
		}
		// constructEigenstrings (:283-317): rows of U
		{
			const real alpha = 0.5;  // normalizer for U1 * U == I
			real pressure = alpha / (c1 * rho);
			for (int r = 0; r < D; r++) m.U[0 * M + r] = n[0][r] * alpha;
			m.U[0 * M + D] = pressure;
			pressure = -pressure;
			for (int r = 0; r < D; r++) m.U[1 * M + r] = n[0][r] * alpha;
			m.U[1 * M + D] = pressure;
			for (int i = 1; i < D; i++) {
				for (int r = 0; r < D; r++) m.U[(i + 1) * M + r] = n[i][r];
				m.U[(i + 1) * M + D] = 0;
			}
		}
		m.checkDecomposition(100 * EQUALITY_TOLERANCE);
	}
};

// ------------------------------------------------- quantities on vectors --
/// AcousticVariables::QUANTITIES (rheology/variables/AcousticVariables.hpp):
/// Vx..V(D-1) and PRESSURE, which is component D itself; -1 for any other
/// quantity (the reference's map lookup throws there).
inline int acousticQuantityComponent(int D, PhysicalQuantities::T q) {
	using Q = PhysicalQuantities::T;
	switch (q) {
	case Q::Vx: return 0;
	case Q::Vy: return D > 1 ? 1 : -1;
	case Q::Vz: return D > 2 ? 2 : -1;
	case Q::PRESSURE: return D;
	default: return -1;
	}
}
inline real getAcousticQuantity(int D, PhysicalQuantities::T q, const real* v) {
	const int c = acousticQuantityComponent(D, q);
	if (c < 0) throw Exception("quantity not present in the acoustic PDE vector");
	return v[c];
}
inline void setAcousticQuantity(int D, PhysicalQuantities::T q, real value, real* v) {
	const int c = acousticQuantityComponent(D, q);
	if (c < 0) throw Exception("quantity not present in the acoustic PDE vector");
	v[c] = value;
}
/// Column of U1 a wave type selects (Model.cpp:55-60): P_FORWARD / P_BACKWARD
/// are columns 0 / 1; the acoustic model has no S waves.
inline int acousticWaveColumn(Waves::T w) {
	if (w == Waves::T::P_FORWARD) return 0;
	if (w == Waves::T::P_BACKWARD) return 1;
	throw Exception("wave type not present in the acoustic model");
}

/// Model-aware forms used where a body of either model passes through.
inline int pdeSizeOf(Models::T model, int D) { return model == Models::T::ACOUSTIC ? acousticPdeSize(D) : pdeSize(D); }
inline bool hasQuantityOf(Models::T model, int D, PhysicalQuantities::T q) {
	return model == Models::T::ACOUSTIC ? acousticQuantityComponent(D, q) >= 0 : hasQuantity(D, q);
}
inline real getQuantityOf(Models::T model, int D, PhysicalQuantities::T q, const real* v) {
	return model == Models::T::ACOUSTIC ? getAcousticQuantity(D, q, v) : getQuantity(D, q, v);
}

}  // namespace gcm
