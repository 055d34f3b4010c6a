// Stand-in for <opencv2/opencv.hpp> (the reference's Sim3Solver.h includes it): see core/core.hpp beside it.
#pragma once
#include "core/core.hpp"
