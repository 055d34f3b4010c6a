#pragma once
#include "../../../g2o_sim3_standin.hpp"
